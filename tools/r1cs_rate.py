#!/usr/bin/env python3
"""Rate of pzk_r1cs_check_batch on one GPU. Builds, with tests/r1cs_ref.py's generator, a local system
of the canonical instance's size (2,251,704 wires and as many constraints, 1 - 3 terms per LC from a window of +-64
wires, one constraint in 512 long with 254 terms), replicates one satisfying row to `batch` rows in HBM and times the
check with HIP events on a caller stream: the median of `launches` launches after `warmup` untimed ones. Prints one
JSON line: witnesses/s, ms per launch, and the algorithmic bytes read per second (32 * n_wires per witness plus the CSR
— terms, LC offsets, chunk table — once per tile of R1CS_WT witnesses).

--oracle N: first time oracle/r1cs_check.c (pyr1cs.check_register, the procedural CPU checker this path is measured
against) on a canonical oracle witness, on 1 process and on N processes, before the GPU is touched.

python tools/r1cs_rate.py [--wires 2251704] [--batch 256] [--launches 15] [--warmup 2] [--general 0.0] [--oracle 16]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "passport-zk-circuits_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "oracle"))

HBM_PEAK_GBS = 8000.0


def _oracle_worker(args):
    """one process: check the witness `reps` times -> seconds per check"""
    path, reps = args
    import numpy as np
    import pyr1cs
    from pzkwit import inputs as I
    wit = np.load(path)
    rc, rep = pyr1cs.check_register(wit, **I.CANONICAL)  # loads the tables; not timed
    assert rc == 0, rep
    t = time.perf_counter()
    for _ in range(reps):
        rc, rep = pyr1cs.check_register(wit, **I.CANONICAL)
        assert rc == 0
    return (time.perf_counter() - t) / reps, int(rep["n_constraints"])


def oracle_rates(nproc, reps=5):
    import multiprocessing as mp
    import tempfile

    import numpy as np
    import pyoracle
    from pzkwit import inputs as I
    g = I.PassportGen(seed=3, n_keys=1, workers=1)
    row = I.pack_register_inputs(g.passport_at(0))
    rc, wit = pyoracle.register_witness(pyoracle.register_params(**I.CANONICAL), row)
    assert rc == 0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "wit.npy")
        np.save(path, wit)
        one, ncons = _oracle_worker((path, reps))
        ctx = mp.get_context("spawn")
        with ctx.Pool(nproc) as pool:
            pool.map(_oracle_worker, [(path, 1)] * nproc)  # start-up and table loads, untimed
            t = time.perf_counter()
            pool.map(_oracle_worker, [(path, reps)] * nproc)
            wall = time.perf_counter() - t
    # each worker runs reps + 1 checks inside the timed map (one untimed by itself, but inside the wall time)
    return dict(oracle_constraints=ncons, oracle_1cpu_s_per_witness=round(one, 3), oracle_1cpu_witnesses_per_s=round(1 / one, 3),
                oracle_nproc=nproc, oracle_nproc_witnesses_per_s=round(nproc * (reps + 1) / wall, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wires", type=int, default=2251704)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--general", type=float, default=None,
                    help="share of coefficients other than +-1 (default: the generator's pool, 15 %%)")
    ap.add_argument("--oracle", type=int, default=0, help="also time the CPU oracle checker on 1 and on N processes")
    args = ap.parse_args()

    out = {}
    if args.oracle:
        out.update(oracle_rates(args.oracle))

    import numpy as np
    import r1cs_ref
    t = time.perf_counter()
    data, wit, _ = r1cs_ref.local_system(args.wires, general=args.general)
    gen_s = time.perf_counter() - t

    import torch
    from pzkwit.r1cs import R1cs

    dev = torch.device("cuda:0")
    torch.cuda.init()
    t = time.perf_counter()
    r = R1cs(data)
    load_s = time.perf_counter() - t
    file_bytes = len(data)
    del data
    info = r.info
    W, B = info["n_wires"], args.batch
    stride = 32 * W
    row = torch.from_numpy(np.frombuffer(wit, dtype=np.uint8).copy()).to(dev)
    d_rows = row.unsqueeze(0).repeat(B, 1).contiguous()
    first = torch.full((B,), 7, dtype=torch.int32, device=dev)
    cnt = torch.full((B,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(device=dev)
    ms = []
    with torch.cuda.stream(s):
        for k in range(args.warmup + args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            r.check_device(d_rows.data_ptr(), B, stride, first.data_ptr(), cnt.data_ptr(), stream=s.cuda_stream, sync=False)
            e1.record(s)
            e1.synchronize()
            if k >= args.warmup:
                ms.append(e0.elapsed_time(e1))
    assert first.cpu().tolist() == [-1] * B and cnt.cpu().tolist() == [0] * B, "the replicated row must satisfy the system"
    # a violated row is still seen at this size: one element of the last row replaced
    d_rows[B - 1, 32 * (W // 2)] ^= 1
    torch.cuda.synchronize(dev)
    r.check_device(d_rows.data_ptr(), B, stride, first.data_ptr(), cnt.data_ptr())
    f = first.cpu().tolist()
    assert f[: B - 1] == [-1] * (B - 1) and f[B - 1] >= 0, f[-3:]

    med = statistics.median(ms)
    n_chunks_bytes = 8 * ((info["n_constraints"] + 255) // 256)
    csr = 8 * info["n_terms"] + 4 * (3 * info["n_constraints"] + 1) + n_chunks_bytes
    tiles = (B + r1cs_ref.R1CS_WT - 1) // r1cs_ref.R1CS_WT
    algo = B * 32 * W + tiles * csr
    out.update(dict(
        metric="r1cs_check_witnesses_per_s", value=round(B / (med / 1e3), 1), ms_per_launch_median=round(med, 3),
        ms_per_launch_min=round(min(ms), 3), ms_per_launch_max=round(max(ms), 3), launches=len(ms), batch=B,
        algorithmic_bytes_per_launch=algo, csr_bytes=csr, read_gb_per_s=round(algo / (med / 1e3) / 1e9, 1),
        hbm_fraction=round(algo / (med / 1e3) / 1e9 / HBM_PEAK_GBS, 4), file_bytes=file_bytes, general_share=0.15 if args.general is None else args.general,
        generate_s=round(gen_s, 1), load_s=round(load_s, 1), first_failed_of_the_damaged_row=f[B - 1], **info))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
