"""GPU: RegisterIdentityBuilder at the edges of its accepted parameter ranges and on rows that fail the
PassportVerificationFlow block one comparison at a time (tests/register_cases.py; the rows are pinned on the oracle
and on a Python restatement of the flow by tests/test_register_cases.py).

One test per instance: the instance is created and all its rows go through witness_batch_host, one call of at most
16 rows (a flow instance: passing, failing, passing, ..., passing, so every failing lane sits between clean ones;
its 16 to 22 failing rows take three or four such calls on the one instance). Every witness element of every row is
compared with the oracle's, failing rows included: the flow only produces booleans, so a failing row leaves every
other signal defined. Statuses are exactly 0, or 7 (PZK_ST_FLOW) where the row was tampered with. The `odd` and
`flow_aa23` rows also go through the packed entry point and must give the same witnesses."""
import time

import numpy as np
import pytest

from pzkwit import native

import register_cases as C
from test_gpu_register import mismatch_report, region_table

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(C.PARAMS))
def test_instance_matches_oracle(oracle, name):
    params, batches = C.batches(name)
    prm = oracle.register_params(**params)
    regions = region_table(params)
    t0 = time.perf_counter()
    inst = native.Instance(native.PZK_CIRCUIT_REGISTER, 0, params)
    t_create = time.perf_counter() - t0
    refs, problems, t_call = {}, [], 0.0
    try:
        for batch in batches:
            assert len(batch) <= C.MAX_BATCH
            rows = np.stack([r.packed for r in batch])
            t0 = time.perf_counter()
            wit, st = inst.witness_batch_host(rows)
            t_call += time.perf_counter() - t0
            packed_wit = None
            if name in C.PACKED_INSTANCES:
                packed, pst = native.pack_inputs(rows, params)
                assert (pst == 0).all(), pst
                packed_wit, packed_st = inst.witness_batch_host_packed(packed)
                assert packed_st.tolist() == st.tolist()
            for b, r in enumerate(batch):
                ref = refs.get(id(r))  # the two passing rows recur: their references are kept, a failing row's is not
                if ref is None:
                    rc, ref = oracle.register_witness(prm, r.packed)
                    assert rc == r.code, (str(r), rc)  # as test_register_cases.py pinned it
                    ref.setflags(write=False)
                    if not r.code:
                        refs[id(r)] = ref
                if int(st[b]) != r.code:
                    problems.append("row %d (%s): status %d, expected %d" % (b, r, st[b], r.code))
                rep = mismatch_report(ref, wit[b], regions)
                if rep:
                    problems.append("row %d (%s): %s" % (b, r, rep))
                if packed_wit is not None and (packed_wit[b] != wit[b]).any():
                    bad = np.nonzero((packed_wit[b] != wit[b]).any(axis=1))[0]
                    problems.append("row %d (%s): %d elements of the packed call differ from the unpacked one, first %d"
                                    % (b, r, bad.size, bad[0]))
    finally:
        inst.close()
    print("%s: %d elements, %d rows in %d calls; instance %.2f s, calls %.2f s" % (
        name, inst.witness_size, sum(len(b) for b in batches), len(batches), t_create, t_call))
    assert not problems, "\n".join(problems[:20])
