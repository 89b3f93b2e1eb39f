"""Checking witness rows against a circom .r1cs file (include/pzkwit.h pzk_r1cs_*): the counterpart of
circom_tester's circuit.checkConstraints(w), for whole batches, on the rows where the GPU wrote them.

    r = R1cs("circuit.r1cs")
    first_failed, n_failed = r.check(witness)        # (batch, n_wires, 32) uint8, through the device
    r.check_device(d_wtns, batch, stride, d_first)   # rows already in HBM (pzk_witness_batch's output)

    h = r.quotient(witness)                          # Groth16's quotient evaluations, (batch, N, 32) uint8
    r.quotient_device(d_wtns, batch, stride, d_h, h_stride)   # the same where the rows lie

first_failed[i] is -1 when row i satisfies every constraint, else the lowest violated constraint index in file order.
eval_host is the kernels' host twin (one thread, no device); check and check_device never fall back to it."""
import ctypes
import os

import numpy as np

from . import native


class R1cs:
    def __init__(self, path_or_bytes):
        if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
            data = bytes(path_or_bytes)
        else:
            with open(os.fspath(path_or_bytes), "rb") as f:
                data = f.read()
        h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
        native._check(native.lib().pzk_r1cs_load(buf, len(data), ctypes.byref(h)))
        self._h = h
        info = native.PzkR1csInfo()
        native._check(native.lib().pzk_r1cs_get_info(h, ctypes.byref(info)))
        self.info = {k: int(getattr(info, k)) for k, _ in native.PzkR1csInfo._fields_}
        self.n_wires = self.info["n_wires"]
        self.n_constraints = self.info["n_constraints"]

    def close(self):
        if getattr(self, "_h", None):
            native.lib().pzk_r1cs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def check_device(self, d_wtns, batch, stride, d_first_failed, d_n_failed=None, stream=None, sync=True, device=-1):
        """pzk_r1cs_check_batch on device pointers (integers): rows batch x stride bytes, results batch x int32 and
        (optional) batch x uint32. stream: a HIP stream handle the check is ordered after and runs on; None: the
        object's own stream (synchronise the rows' writer first)."""
        ex = native.PzkExec(device=device, flags=native.PZK_EXEC_SYNC if sync else 0, stream=stream)
        native._check(native.lib().pzk_r1cs_check_batch(
            self._h, ctypes.c_void_p(d_wtns), batch, stride, ctypes.c_void_p(d_first_failed),
            ctypes.c_void_p(d_n_failed) if d_n_failed else None, ctypes.byref(ex)))

    def _rows(self, witness):
        a = np.ascontiguousarray(witness, dtype=np.uint8)
        if a.ndim == 2:
            a = a[None]
        assert a.ndim == 3 and a.shape[1] >= self.n_wires and a.shape[2] == 32, a.shape
        return a, a.shape[0], 32 * a.shape[1]

    def check(self, witness):
        """(batch, W >= n_wires, 32) uint8 -> (first_failed (batch,) int32, n_failed (batch,) uint32), on the GPU."""
        a, b, stride = self._rows(witness)
        first, n = np.full(b, -1, dtype=np.int32), np.zeros(b, dtype=np.uint32)
        ex = native.PzkExec(device=-1, flags=0, stream=None)
        native._check(native.lib().pzk_r1cs_check_batch_host(self._h, a.ctypes.data, b, stride, first.ctypes.data,
                                                             n.ctypes.data, ctypes.byref(ex)))
        return first, n

    def eval_host(self, witness):
        """The same through pzk_r1cs_eval_host (plain C++, no device)."""
        a, b, stride = self._rows(witness)
        first, n = np.full(b, -1, dtype=np.int32), np.zeros(b, dtype=np.uint32)
        native._check(native.lib().pzk_r1cs_eval_host(self._h, a.ctypes.data, b, stride, first.ctypes.data,
                                                      n.ctypes.data))
        return first, n

    # ---- Groth16's quotient evaluations (pzk_r1cs_quotient_*)
    def quotient_info(self):
        """{log2_n, tile, n, n_rows, scratch_bytes} of the quotient's domain (host only)"""
        info = native.PzkQuotientInfo()
        native._check(native.lib().pzk_r1cs_quotient_info(self._h, ctypes.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in native.PzkQuotientInfo._fields_}

    def quotient_device(self, d_wtns, batch, stride, d_h, h_stride, stream=None, sync=True, device=-1, timing=False):
        """pzk_r1cs_quotient_batch on device pointers (integers): rows batch x stride bytes in, batch x h_stride bytes
        (>= 32 N) out. stream as for check_device."""
        ex = native.PzkExec(device=device, flags=(native.PZK_EXEC_SYNC if sync else 0) | (2 if timing else 0), stream=stream)
        native._check(native.lib().pzk_r1cs_quotient_batch(self._h, ctypes.c_void_p(d_wtns), batch, stride,
                                                           ctypes.c_void_p(d_h), h_stride, ctypes.byref(ex)))

    def quotient_timing(self, reset=False):
        """ms of the stages of calls made with timing=True: [rows a b c, inverse x 3, forward a b, forward c + pointwise]"""
        ms = (ctypes.c_double * 4)()
        native._check(native.lib().pzk_r1cs_quotient_timing(self._h, ms, 1 if reset else 0))
        return list(ms)

    def quotient(self, witness):
        """(batch, W >= n_wires, 32) uint8 -> h (batch, N, 32) uint8, on the GPU."""
        a, b, stride = self._rows(witness)
        n = self.quotient_info()["n"]
        h = np.zeros((b, n, 32), dtype=np.uint8)
        ex = native.PzkExec(device=-1, flags=0, stream=None)
        native._check(native.lib().pzk_r1cs_quotient_batch_host(self._h, a.ctypes.data, b, stride, h.ctypes.data, 32 * n,
                                                                ctypes.byref(ex)))
        return h

    def quotient_host(self, witness):
        """The same through pzk_r1cs_quotient_host (plain C++, no device)."""
        a, b, stride = self._rows(witness)
        n = self.quotient_info()["n"]
        h = np.zeros((b, n, 32), dtype=np.uint8)
        native._check(native.lib().pzk_r1cs_quotient_host(self._h, a.ctypes.data, b, stride, h.ctypes.data, 32 * n))
        return h
