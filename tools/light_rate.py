#!/usr/bin/env python3
"""Rate of RegisterIdentityLight(DG_HASH_TYPE, DOCUMENT_TYPE) witnesses on one GPU, measured the way bench.py measures
its lines: W untimed warm-up steps, then K timed steps of one batch each between device synchronisations, the rows
written to device memory (host delivery is not timed). Prints one JSON line: witnesses/s and the README's "job HBM"
(algorithmic .wtns + input bytes x witnesses/s / 8 TB/s), with the per-phase kernel times of the timed steps
(PZK_EXEC_TIMING) beside each phase's algorithmic bytes.

python tools/light_rate.py [--batch 4096] [--steps 3] [--warmup 1] [--dg-hash 256] [--doc 3] [--sub N]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "passport-zk-circuits_amd"))

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dg-hash", type=int, default=256)
    ap.add_argument("--doc", type=int, default=3)
    ap.add_argument("--sub", type=int, default=None, help="witnesses per call (default: the whole batch if it fits)")
    args = ap.parse_args()

    import torch
    from pzkwit import light, native

    dev = torch.device("cuda:0")
    torch.cuda.init()
    inst = native.Instance(native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=args.dg_hash, doc=args.doc))
    W, NIN = inst.witness_size, inst.n_inputs
    stride = 32 * W
    rows = light.batch_rows(args.batch, 0x11, args.dg_hash, args.doc)
    d_in = torch.from_numpy(rows).to(dev)
    if args.sub:
        sub = min(args.sub, args.batch)
    else:
        free, _ = torch.cuda.mem_get_info(dev)
        fit = max(1, int(free * 0.85 // (stride + (1 << 20))))
        parts = 1
        while (args.batch + parts - 1) // parts > fit:
            parts += 1
        sub = (args.batch + parts - 1) // parts
    sub = min(sub, 32768)
    d_out = torch.empty(sub * stride, dtype=torch.uint8, device=dev)
    d_st = torch.zeros((max(args.steps, 1), args.batch), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # the library's streams do not wait for torch's stream

    def step(k, timing):
        for lo in range(0, args.batch, sub):
            n = min(sub, args.batch - lo)
            inst.witness_batch_device(d_in.data_ptr() + lo * NIN * 32, n, d_out.data_ptr(), stride,
                                      d_st[k].data_ptr() + 4 * lo, timing=timing)

    for _ in range(args.warmup):
        step(0, False)
    inst.sync()
    inst.timing(reset=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k, True)
    inst.sync()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0

    value = args.batch * args.steps / dt
    job_bytes = 32 * NIN + 76 + 32 * W
    job_gbs = value * job_bytes / 1e9
    tm = inst.timing()
    phases = {}
    for name, kernel, nbytes in inst.phase_info():
        ms, launches = tm.get(name, (0.0, 0))
        if launches:
            per = ms / launches
            phases[name] = {"kernel": kernel, "ms_per_call": round(per, 3), "alg_bytes_per_witness": nbytes,
                            "gbs": round(nbytes * args.batch * args.steps / launches / (per / 1e3) / 1e9, 1) if per else None}
    bad = int((d_st[:args.steps] != 0).sum().item())
    print(json.dumps({
        "metric": "RegisterIdentityLight(%d, %d) witnesses/s" % (args.dg_hash, args.doc), "value": round(value, 2),
        "unit": "witnesses/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "config": {"batch": args.batch, "sub_batch": sub, "witness_elements": W, "witness_bytes": 32 * W,
                   "invalid_lanes": bad},
        "job_hbm": {"alg_bytes_per_witness": job_bytes, "achieved": round(job_gbs, 1), "unit": "GB/s",
                    "frac": round(job_gbs / HBM_PEAK_GBS, 4)},
        "phases": phases}))
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
