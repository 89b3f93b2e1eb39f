#!/usr/bin/env python3
"""Measurements of the packed input path, one JSON line per mode:

  kernel    k_unpack_inputs through pzk_unpack_inputs, timed with HIP events at --batch witnesses for config 3, the
            query and Light, beside a device-to-device hipMemcpyAsync of the same batch x n_inputs x 32 bytes (the copy
            moves twice the HBM traffic: it reads what it writes)
  lines     bench.py-style rates (W warm-up steps, K timed steps between synchronisations) of config 3 at O0, config 3
            under the --sym o2shape map and the query, device-resident inputs, alternating unpacked and packed runs
  hostfed   the same lines fed from pinned host memory: one host-to-device copy per call on the caller's stream, then
            the call, with full rows and with packed rows
  passport  microseconds per passport, one thread, of pzk_passport_inputs and pzk_passport_inputs_packed (no GPU)

python tools/packed_rate.py kernel|lines|hostfed|passport [--batch 4096] [--steps 3] [--warmup 1] [--reps 3]
                                                          [--lines config3,o2shape,query]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "passport-zk-circuits_amd"))
sys.path.insert(1, REPO)  # bench.py's input generators


def line_spec(name):
    """-> (circuit, size_arg, params, sym text or None)"""
    from pzkwit import inputs as I, native, symmap
    if name == "config3":
        return native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL, None
    if name == "o2shape":
        return native.PZK_CIRCUIT_REGISTER, 0, I.CANONICAL, symmap.sym_text_wit(symmap.load_shape("register_canonical", 2))
    if name == "query":
        return native.PZK_CIRCUIT_QUERY, 80, {"doc": 0}, None
    if name == "light":
        return native.PZK_CIRCUIT_LIGHT, 0, dict(dg_hash=256, doc=3), None
    raise SystemExit("unknown line %s" % name)


def line_rows(name, batch, distinct=256):
    """the line's bench.py inputs: `distinct` generated rows repeated along the batch"""
    if name in ("config3", "o2shape"):
        import bench
        uniq = bench.make_register_inputs(min(batch, distinct), 0, seed=3, sig=1, workers=min(16, os.cpu_count() or 1))
    elif name == "query":
        from pzkwit import query as Q
        uniq = Q.batch_rows(min(batch, 64), seed=0x9, distinct=64)
    else:
        from pzkwit import light
        uniq = light.batch_rows(min(batch, 64), 0x11, 256, 3)
    return uniq[np.arange(batch) % uniq.shape[0]]


def pack(name, rows):
    from pzkwit import native
    circuit, size, params, _ = line_spec(name)
    packed, st = native.pack_inputs(rows, params, circuit, size)
    assert (st == 0).all()
    return packed


def mode_kernel(args):
    import torch
    from pzkwit import native
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    dev = torch.device("cuda:0")
    s = torch.cuda.Stream(device=dev)
    out = {"mode": "kernel", "batch": args.batch, "device": torch.cuda.get_device_name(0), "lines": {}}
    for name in ("config3", "query", "light"):
        circuit, size, params, _ = line_spec(name)
        inst = native.Instance(circuit, size, params)
        B = args.batch
        nbytes = B * inst.n_inputs * 32
        d_packed = torch.from_numpy(pack(name, line_rows(name, B, 64))).to(dev)
        d_rows = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d_src = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def unpack():
            inst.unpack_inputs_device(d_packed.data_ptr(), B, d_rows.data_ptr(), stream=s.cuda_stream, sync=False)

        def copy():
            assert hip.hipMemcpyAsync(d_rows.data_ptr(), d_src.data_ptr(), nbytes, 3, s.cuda_stream) == 0

        res = {}
        for label, fn in (("unpack", unpack), ("d2d_copy", copy)):
            for _ in range(3):
                fn()
            s.synchronize()
            ms = []
            for _ in range(args.reps * 5):  # one launch per event pair, the median of them
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                fn()
                e1.record(s)
                s.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            res[label] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                          "written_TBps": round(nbytes / med / 1e9, 3)}
        res["bytes_written"] = nbytes
        res["packed_bytes_read"] = int(d_packed.numel())
        out["lines"][name] = res
        inst.close()
        del d_packed, d_rows, d_src
        torch.cuda.empty_cache()
    print(json.dumps(out))


class Line:
    """one line's instance and inputs, bench.py's sub-batching (one output slot per stream in use)"""

    def __init__(self, name, args, slots=1):
        import torch
        from pzkwit import native
        self.torch, self.name, self.args = torch, name, args
        circuit, size, params, sym = line_spec(name)
        self.dev = torch.device("cuda:0")
        self.inst = native.Instance(circuit, size, params, sym=sym)
        self.W, self.NIN, self.PB = self.inst.witness_size, self.inst.n_inputs, self.inst.packed_row_bytes
        self.batch, self.stride, self.slots = args.batch, 32 * self.inst.witness_size, slots
        self.rows = line_rows(name, self.batch)
        self.packed = pack(name, self.rows)
        free, _ = torch.cuda.mem_get_info(self.dev)
        staging = 2 * 1024 * 32 * int(native.layout_info(params, circuit, size).witness_size) if sym else 0
        fit = max(1, int((free * 0.8 - staging) // (slots * self.stride + (2 << 20) + 64 * self.NIN)))
        parts = 1
        while (self.batch + parts - 1) // parts > fit:
            parts += 1
        self.sub = min((self.batch + parts - 1) // parts, 32768)
        self.d_out = torch.empty(slots * self.sub * self.stride, dtype=torch.uint8, device=self.dev)
        self.d_st = torch.zeros(self.batch, dtype=torch.int32, device=self.dev)

    def timed(self, step):
        a = self.args
        for _ in range(a.warmup):
            step()
        self.inst.sync()
        self.torch.cuda.synchronize(self.dev)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        self.inst.sync()
        self.torch.cuda.synchronize(self.dev)
        dt = time.perf_counter() - t0
        assert int((self.d_st != 0).sum().item()) == 0
        return self.batch * a.steps / dt


def mode_lines(args):
    import torch
    out = {"mode": "lines", "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "lines": {}}
    for name in args.lines.split(","):
        L = Line(name, args)
        d_full = torch.from_numpy(L.rows).to(L.dev)
        d_packed = torch.from_numpy(L.packed).to(L.dev)
        torch.cuda.synchronize()

        def step(packed):
            for lo in range(0, L.batch, L.sub):
                n = min(L.sub, L.batch - lo)
                if packed:
                    L.inst.witness_batch_packed_device(d_packed.data_ptr() + lo * L.PB, n, L.d_out.data_ptr(), L.stride,
                                                       L.d_st.data_ptr() + 4 * lo)
                else:
                    L.inst.witness_batch_device(d_full.data_ptr() + lo * L.NIN * 32, n, L.d_out.data_ptr(), L.stride,
                                                L.d_st.data_ptr() + 4 * lo)

        runs = {"unpacked": [], "packed": []}
        for _ in range(args.reps):  # alternating
            runs["unpacked"].append(round(L.timed(lambda: step(False)), 1))
            runs["packed"].append(round(L.timed(lambda: step(True)), 1))
        out["lines"][name] = {"sub_batch": L.sub, "witness_bytes": L.stride, "row_bytes": 32 * L.NIN,
                              "packed_row_bytes": L.PB, "witnesses_per_s": runs,
                              "median": {k: statistics.median(v) for k, v in runs.items()}}
        L.inst.close()
        del L, d_full, d_packed
        torch.cuda.empty_cache()
    print(json.dumps(out))


def mode_hostfed(args):
    import torch
    NS = 2  # caller streams (and output slots, device input buffers): one call's upload beside the other's kernels
    out = {"mode": "hostfed", "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "caller_streams": NS,
           "device": torch.cuda.get_device_name(0), "lines": {}}
    for name in args.lines.split(","):
        L = Line(name, args, slots=NS)
        streams = [torch.cuda.Stream(device=L.dev) for _ in range(NS)]
        h = {"unpacked": torch.from_numpy(L.rows.reshape(L.batch, -1)).pin_memory(),
             "packed": torch.from_numpy(L.packed).pin_memory()}
        d_in = {k: [torch.empty((L.sub, v.shape[1]), dtype=torch.uint8, device=L.dev) for _ in range(NS)]
                for k, v in h.items()}
        torch.cuda.synchronize()

        def step(kind):
            for j, lo in enumerate(range(0, L.batch, L.sub)):
                n, k = min(L.sub, L.batch - lo), j % NS
                s = streams[k]
                with torch.cuda.stream(s):
                    d_in[kind][k][:n].copy_(h[kind][lo:lo + n], non_blocking=True)  # one H2D copy per call
                fn = L.inst.witness_batch_packed_device if kind == "packed" else L.inst.witness_batch_device
                fn(d_in[kind][k].data_ptr(), n, L.d_out.data_ptr() + k * L.sub * L.stride, L.stride,
                   L.d_st.data_ptr() + 4 * lo, stream=s.cuda_stream)

        runs = {"unpacked": [], "packed": []}
        for _ in range(args.reps):
            for kind in ("unpacked", "packed"):
                runs[kind].append(round(L.timed(lambda: step(kind)), 1))
        out["lines"][name] = {"sub_batch": L.sub, "row_bytes": 32 * L.NIN, "packed_row_bytes": L.PB,
                              "witnesses_per_s": runs, "median": {k: statistics.median(v) for k, v in runs.items()},
                              "upload_GBps_at_median": {k: round(statistics.median(v) * h[k].shape[1] / 1e9, 2)
                                                        for k, v in runs.items()}}
        L.inst.close()
        del L, h, d_in
        torch.cuda.empty_cache()
    print(json.dumps(out))


def mode_passport(args):
    from pzkwit import passport as PP, sodgen
    key = sodgen.signer_key(1)
    uniq = [sodgen.make_passport(1, key, i) for i in range(64)]
    n = min(args.batch, 2048)
    batch = [uniq[i % len(uniq)] for i in range(n)]
    params = PP.parse(batch[0])["params"]
    srcs = PP.sources(batch)
    bufs = {"full": PP.input_rows(params, batch[:1])[0], "packed": PP.packed_rows(params, batch[:1])[0]}
    res = {"mode": "passport", "passports": n, "threads": 1, "us_per_passport": {}}
    for kind, fn in (("full", PP.input_rows), ("packed", PP.packed_rows)):
        rows = np.ones((n,) + bufs[kind].shape[1:], dtype=np.uint8)  # pages faulted in
        us = []
        for _ in range(args.reps):
            t = time.perf_counter()
            _, st = fn(params, srcs, threads=1, out=rows)
            us.append((time.perf_counter() - t) / n * 1e6)
            assert (st == 0).all()
        res["us_per_passport"][kind] = {"runs": [round(u, 2) for u in us], "median": round(statistics.median(us), 2),
                                        "row_bytes": int(rows[0].size)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "lines", "hostfed", "passport"])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3, help="runs of each kind (lines, hostfed, passport)")
    ap.add_argument("--lines", default="config3,o2shape,query")
    args = ap.parse_args()
    {"kernel": mode_kernel, "lines": mode_lines, "hostfed": mode_hostfed, "passport": mode_passport}[args.mode](args)


if __name__ == "__main__":
    main()
