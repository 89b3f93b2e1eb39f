#!/usr/bin/env python3
"""Rate of pzk_r1cs_quotient_batch on one GPU, the counterpart of tools/r1cs_rate.py: the same local
system of the canonical instance's size (2,251,704 wires and as many constraints: M = 2,251,705 rows, N = 2^22), one
satisfying row replicated to `batch` rows in HBM, the call timed with HIP events on a caller stream: the median of
`launches` launches after `warmup` untimed ones. Then `stage_launches` launches with PZK_EXEC_TIMING for the
milliseconds per stage (the rows a, b, c; the three inverse transforms with the shift; the forward transforms of a and
b; the forward transform of c with the pointwise step folded into its last pass). Prints one JSON line with
witnesses/s, ms per launch and per stage, and the bytes and field products the algorithm needs per row, so that the
rate can be set against the store / stream ceilings and the measured product rates of DESIGN.md §4.2.

--host: also run the host twin (pzk_r1cs_quotient_host, one thread) on the row, time it, and compare the device's h
byte for byte with it. Without it the device rows are only compared with each other (they are replicas).

--cache PATH: keep the generated system in PATH (.npz) and read it from there when it exists.

python tools/quotient_rate.py [--wires 2251704] [--batch 16] [--launches 10] [--warmup 2] [--stage-launches 2] [--host]
                              [--cache PATH]
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

NTT_R = 10  # csrc/ntt.hpp


def counts(k, n_wires, n_constraints):
    """algorithmic bytes and Montgomery products per row, from the shapes (csrc/ntt.hpp, kernels_quotient.hip)"""
    n = 1 << k
    passes = -(-k // NTT_R)
    vec = 32 * n
    by = dict(ab=32 * n_wires + 3 * vec,                       # the row read once (gathers), a, b, c written
              transforms=6 * passes * 2 * vec,                  # each pass reads and writes a vector
              pointwise=2 * vec)                                # the folded pass also reads a' and b'
    # a stage with unit roots (the first of each forward pass, the last of each inverse pass) has no product
    pr = dict(butterflies=6 * (n // 2) * (k - passes),
              between_passes=3 * 2 * n * passes + 3 * 2 * n * (passes - 1),  # two-level factors: 2 products per element
              pointwise=2 * n,                                  # a' b' and the conversion out of Montgomery form
              ab=3 * n_constraints)
    return passes, by, pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wires", type=int, default=2251704)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stage-launches", type=int, default=2)
    ap.add_argument("--cache", default=None, help="an .npz file that keeps the generated system between runs")
    ap.add_argument("--host", action="store_true", help="time the host twin on one row and compare the device's h with it")
    args = ap.parse_args()

    import numpy as np
    import r1cs_ref
    t = time.perf_counter()
    if args.cache and os.path.exists(args.cache):
        z = np.load(args.cache)
        data, wit = z["data"].tobytes(), z["wit"].tobytes()
        assert len(wit) == 32 * args.wires, "the cached system has another size"
    else:
        data, wit, _ = r1cs_ref.local_system(args.wires)
        if args.cache:
            np.savez(args.cache, data=np.frombuffer(data, dtype=np.uint8), wit=np.frombuffer(wit, dtype=np.uint8))
    gen_s = time.perf_counter() - t

    import torch
    from pzkwit.r1cs import R1cs

    dev = torch.device("cuda:0")
    torch.cuda.init()
    r = R1cs(data)
    del data
    info, qi = r.info, r.quotient_info()
    W, B, k, N = info["n_wires"], args.batch, qi["log2_n"], qi["n"]
    stride, h_stride = 32 * W, 32 * N
    row_np = np.frombuffer(wit, dtype=np.uint8).copy()
    d_rows = torch.from_numpy(row_np).to(dev).unsqueeze(0).repeat(B, 1).contiguous()
    d_h = torch.zeros((B, h_stride), dtype=torch.uint8, device=dev)
    first = torch.full((1,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    r.check_device(d_rows.data_ptr(), 1, stride, first.data_ptr())
    assert first.cpu().tolist() == [-1], "the row must satisfy the system"
    s = torch.cuda.Stream(device=dev)
    ms = []
    with torch.cuda.stream(s):
        for i in range(args.warmup + args.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            r.quotient_device(d_rows.data_ptr(), B, stride, d_h.data_ptr(), h_stride, stream=s.cuda_stream, sync=False)
            e1.record(s)
            e1.synchronize()
            if i >= args.warmup:
                ms.append(e0.elapsed_time(e1))
        r.quotient_timing(reset=True)
        for _ in range(args.stage_launches):
            r.quotient_device(d_rows.data_ptr(), B, stride, d_h.data_ptr(), h_stride, stream=s.cuda_stream, sync=True, timing=True)
        stage = [x / (max(args.stage_launches, 1) * B) for x in r.quotient_timing(reset=True)]
    assert all(torch.equal(d_h[0], d_h[i]) for i in range(1, B)), "replicated rows gave different h"
    assert bool((d_h[0] != 0).any()), "h is all zero"

    out = {}
    if args.host:
        t = time.perf_counter()
        h_host = r.quotient_host(row_np.reshape(1, W, 32))
        out["host_1cpu_s_per_row"] = round(time.perf_counter() - t, 2)
        out["device_equals_host_twin"] = bool(np.array_equal(h_host.reshape(-1), d_h[0].cpu().numpy()))
        assert out["device_equals_host_twin"]

    med = statistics.median(ms)
    passes, by, pr = counts(k, W, info["n_constraints"])
    row_ms = med / B
    out.update(dict(
        metric="r1cs_quotient_witnesses_per_s", value=round(B / (med / 1e3), 1), ms_per_launch_median=round(med, 2),
        ms_per_launch_min=round(min(ms), 2), ms_per_launch_max=round(max(ms), 2), launches=len(ms), batch=B, log2_n=k,
        passes=passes, ms_per_row=round(row_ms, 3),
        stage_ms_per_row=dict(zip(("ab", "inverse_x3", "forward_a_b", "forward_c_pointwise"), (round(x, 3) for x in stage))),
        pointwise_ms_per_row_by_difference=round(stage[3] - stage[2] / 2, 3),
        bytes_per_row=by, bytes_per_row_total=sum(by.values()), tb_per_s=round(sum(by.values()) / (row_ms / 1e3) / 1e12, 3),
        products_per_row=pr, products_per_row_total=sum(pr.values()),
        g_products_per_s=round(sum(pr.values()) / (row_ms / 1e3) / 1e9, 1),
        scratch_bytes=qi["scratch_bytes"], generate_s=round(gen_s, 1), n_wires=W, n_constraints=info["n_constraints"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
