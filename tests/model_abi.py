"""The backends of the synthetic-weight model tests (tests/model_cases.py holds the cases and the checks): the library's C ABI on host
buffers (the emulated library) or on GPU buffers, and on the GPU the Python front ends.  TEST INFRASTRUCTURE.

A backend runs the kernels: cell(blob, C, x, hx0, mode) -> (out, hx), mode in "fp32" / "bf16" / ("ex", scale) and, GpuBackend only, "module" /
"module-bf16" (GRUUNet2.forward); momo(blob, pads, x, hx0, prev, via) -> (out, hx, last frame), via in "abi" / "module";
momo_status(...) -> the status dn_momo_forward returns for a shape; process_frame(p, frames, hx0) -> (mel residual, hx);
chain(path, signal) -> hx after mc.CHAIN_HOPS hops.
"""
import ctypes as C

import numpy as np
import torch

import model_cases as mc

class Abi:
    """The library's C ABI with buffers on the host (the emulated library: device = None) or on a GPU (torch tensors on `device`).  Launches go to
    the null stream, which torch's copies order after."""

    def __init__(self, lib, device=None):
        self.lib, self.device = lib, device

    def up(self, a, dtype=np.float32):
        a = np.array(a, dtype=dtype, order="C")
        return a if self.device is None else torch.from_numpy(a).to(self.device)

    def nan(self, *shape):
        return self.up(np.full(shape, np.nan, np.float32))

    def ptr(self, t):
        if t is None:
            return None
        return t.ctypes.data_as(C.c_void_p) if isinstance(t, np.ndarray) else C.c_void_p(t.data_ptr())

    def down(self, t):
        return t if isinstance(t, np.ndarray) else t.cpu().numpy()

    # -- the model kernels
    def model(self, blob, Cb):
        from audio_denoising_amd._lib import ModelCfg
        blob = np.ascontiguousarray(blob, np.float32)
        m = C.c_void_p()
        self.lib.check(self.lib.dn_model_create(blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(ModelCfg(Cb, 1, 4, 17, 3, 2, 1, 6)), C.byref(m)))
        return m

    def cell(self, blob, Cb, x, hx0, mode):
        lib = self.lib
        B, T, F = x.shape
        m = self.model(blob, Cb)
        out, hx1, xd, hd = self.nan(B, T, F), self.nan(B, 17, Cb), self.up(x), self.up(hx0)      # (every buffer stays referenced until read back)
        args = (m, self.ptr(xd), self.ptr(hd), self.ptr(out), self.ptr(hx1), B, T, F, Cb)
        if mode == "fp32":
            lib.check(lib.dn_cell_forward(*args, None))
        elif mode == "bf16":
            lib.check(lib.dn_cell_forward_bf16(*args, None))
        else:
            assert mode[0] == "ex", mode
            lib.check(lib.dn_cell_forward_ex(*args, C.c_float(mode[1]), None))
        res = self.down(out), self.down(hx1)
        lib.dn_model_destroy(m)
        return res

    def momo(self, blob, pads, x, hx0, prev, via="abi"):
        from audio_denoising_amd._lib import MomoCfg
        lib = self.lib
        B, T, F = x.shape
        Cb = hx0.shape[2]
        blob = np.ascontiguousarray(blob, np.float32)
        h = C.c_void_p()
        lib.check(lib.dn_momo_create(blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(MomoCfg(Cb, 1, 3, 16, 3, 2, (C.c_int32 * 3)(*pads), 6)),
                                     C.byref(h)))
        out, hx1, last = self.nan(B, T, F), self.nan(B, 16, Cb), self.nan(B, F)
        p, xd, hd = None if prev is None else self.up(prev.reshape(B, F)), self.up(x), self.up(hx0)
        lib.check(lib.dn_momo_forward(h, self.ptr(xd), self.ptr(hd), self.ptr(p), self.ptr(out), self.ptr(hx1), self.ptr(last), B, T, F, Cb, None))
        res = self.down(out), self.down(hx1), self.down(last)
        lib.dn_momo_destroy(h)
        return res

    def momo_status(self, pads, F, Cb, B=1, T=1):
        """the status dn_momo_forward returns for an input of F bins and an hx of Cb compressed bins (zero inputs)"""
        from audio_denoising_amd._lib import MomoCfg
        lib = self.lib
        blob = np.ascontiguousarray(mc.synth_weights.momo3_blob(0), np.float32)
        h = C.c_void_p()
        lib.check(lib.dn_momo_create(blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(MomoCfg(Cb, 1, 3, 16, 3, 2, (C.c_int32 * 3)(*pads), 6)),
                                     C.byref(h)))
        x, hx0, out, hx1 = self.up(np.zeros((B, T, F))), self.up(np.zeros((B, 16, Cb))), self.nan(B, T, F), self.nan(B, 16, Cb)
        rc = lib.dn_momo_forward(h, self.ptr(x), self.ptr(hx0), None, self.ptr(out), self.ptr(hx1), None, B, T, F, Cb, None)
        msg = lib.dn_last_error() if rc else b""
        lib.dn_momo_destroy(h)
        return rc, msg

    # -- cell_body inside the hop kernels
    def dsp(self, p):
        from audio_denoising_amd._lib import DspCfg
        fb, w = np.ascontiguousarray(mc.hop_fbank(p), np.float32), np.ascontiguousarray(mc.hop_window(p.n_fft), np.float32)
        # 80 mels on the 257 bins of n_fft 512 leave filters empty: the plan then wants the pseudo-inverse from the caller (it feeds the stages
        # behind the model, which are not compared here)
        pinv = None if np.linalg.matrix_rank(fb) == p.n_mels else np.ascontiguousarray(np.linalg.pinv(fb.astype(np.float64).T), np.float32)
        d = C.c_void_p()
        self.lib.check(self.lib.dn_dsp_create(C.byref(DspCfg(p.sample_rate, p.n_fft, p.hop, p.n_mels)), fb.ctypes.data_as(C.c_void_p),
                                              None if pinv is None else pinv.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), C.byref(d)))
        return d

    def workspace(self, dsp, B):
        return self.up(np.zeros(self.lib.dn_workspace_bytes(dsp, B) // 4 + 16, np.float32))

    def process_frame(self, p, frames, hx0):
        """dn_process_frame -> (mel residual (B, 3, M), hx)"""
        lib, B = self.lib, frames.shape[0]
        dsp, m = self.dsp(p), self.model(mc.hop_blob(), p.num_compressed_bins)
        hx, out, resid, ws, fr = self.up(hx0), self.nan(B, p.n_fft), self.nan(B, 3, p.n_mels), self.workspace(dsp, B), self.up(frames)
        lib.check(lib.dn_process_frame(m, dsp, self.ptr(fr), self.ptr(hx), self.ptr(out), self.ptr(resid), None, 11, 3, mc.HOP_N_ITER, 0.99,
                                       self.ptr(ws), B, 0, None))
        res = self.down(resid), self.down(hx)
        assert np.isfinite(self.down(out)).all()
        lib.dn_model_destroy(m)
        lib.dn_dsp_destroy(dsp)
        return res

    def chain(self, path, signal):
        """mc.CHAIN_HOPS consecutive hops of `signal` (B, n_fft + (mc.CHAIN_HOPS - 1) hop) at mc.CHAIN_P through one of mc.CHAIN_PATHS, hx starting at zero
        -> the hx the path leaves behind"""
        from audio_denoising_amd import _lib as L
        lib, p, n = self.lib, mc.CHAIN_P, mc.CHAIN_HOPS
        B = signal.shape[0]
        dsp, m = self.dsp(p), self.model(mc.hop_blob(), p.num_compressed_bins)
        hx = self.up(np.zeros((B, 17, p.num_compressed_bins), np.float32))
        frames = np.stack([signal[:, h * p.hop:h * p.hop + p.n_fft] for h in range(n)])
        hops = [signal[:, k * p.hop:(k + 1) * p.hop] for k in range(n + 1)]            # hop 0 primes the ring of the streaming paths
        if path in ("group", "split"):
            pipe = C.c_void_p()
            lib.check(lib.dn_pipe_create(m, dsp, B, 0, C.byref(pipe)))
            fr, out = self.up(frames), self.nan(n, B, p.n_fft)
            if path == "group":
                lib.check(lib.dn_pipe_set_group(pipe, mc.CHAIN_GROUP))
                for h0 in range(0, n, mc.CHAIN_GROUP):
                    k = min(mc.CHAIN_GROUP, n - h0)
                    lib.check(lib.dn_pipe_submit_group(pipe, self.ptr(fr[h0:]), B * p.n_fft, self.ptr(hx), self.ptr(out[h0:]), B * p.n_fft, None, 0,
                                                       11, 3, k, mc.HOP_N_ITER, 0.99, None))
            else:
                lib.check(lib.dn_pipe_set_head_start(pipe, 0))                     # (a split hop cannot carry a head start)
                lib.check(lib.dn_pipe_set_split(pipe, L.DN_SPLIT_ON))
                for h in range(n):
                    lib.check(lib.dn_pipe_submit(pipe, self.ptr(fr[h]), self.ptr(hx), self.ptr(out[h]), None, 11, 3, mc.HOP_N_ITER, 0.99, None))
            lib.check(lib.dn_pipe_flush(pipe, mc.HOP_N_ITER, 0.99, None))
            assert np.isfinite(self.down(out)).all()
            res = self.down(hx)
            lib.dn_pipe_destroy(pipe)
        elif path in ("sessions", "sessions_two_launches"):
            from audio_denoising_amd.sessions import SessionState
            pool = C.c_void_p()
            lib.check(lib.dn_sessions_create(m, dsp, B + 1, 0, C.byref(pool)))
            if path == "sessions_two_launches":
                lib.check(lib.dn_sessions_set_schedule(pool, 2))          # DN_SESS_TWO_LAUNCHES (the default at this list size: one launch)
            ids = np.ascontiguousarray(np.arange(B, 0, -1), np.int32)                  # streams on slots B .. 1
            idp = ids.ctypes.data_as(C.c_void_p)
            lib.check(lib.dn_sessions_open(pool, idp, B, None, None))
            hin, outs = [self.up(h) for h in hops], [self.nan(B, p.hop) for _ in hops]
            for k in range(n + 1):
                lib.check(lib.dn_sessions_push(pool, idp, B, self.ptr(hin[k]), 0, self.ptr(outs[k]), 0, None, 11, mc.HOP_N_ITER, 0.99, None))
            assert all(np.isfinite(self.down(o)).all() for o in outs)
            rec = self.up(np.zeros((B, int(lib.dn_sessions_record_bytes(pool))), np.uint8), np.uint8)
            lib.check(lib.dn_sessions_export(pool, idp, B, self.ptr(rec), None))
            st = SessionState.from_records(self.down(rec), seed=11)
            assert st.frames.tolist() == [n] * B
            res = np.array(st.hx)
            lib.dn_sessions_destroy(pool)
        else:
            assert path == "clip", path
            ring = np.zeros((B, p.n_fft), np.float32)
            ring[:, p.hop:] = hops[0]
            ring, ola, out = self.up(ring), self.up(np.zeros((B, p.n_fft), np.float32)), self.nan(B, n * p.hop)
            ws, hin = self.up(np.zeros(lib.dn_clip_workspace_bytes(dsp, B, n) // 4, np.float32)), self.up(np.concatenate(hops[1:], axis=1))
            lib.check(lib.dn_clip_process(m, dsp, self.ptr(hin), 0, self.ptr(ring), self.ptr(ola), self.ptr(hx),
                                          self.ptr(out), 0, None, 11, 3, mc.HOP_N_ITER, 0.99, self.ptr(ws), B, n, 0, None))
            assert np.isfinite(self.down(out)).all()
            res = self.down(hx)
        lib.dn_model_destroy(m)
        lib.dn_dsp_destroy(dsp)
        return res


class GpuBackend(Abi):
    """Abi on cuda:0 plus the Python front ends: GRUUNet2.forward (built for 5 compressed bins, run at the C of hx), conv_precision "bf16",
    MOMO3.forward, Denoiser.process_frame"""

    def __init__(self):
        from audio_denoising_amd import _lib
        super().__init__(_lib.get_lib(), torch.device("cuda:0"))

    def gruunet2(self, blob):
        from audio_denoising_amd.gruunet2 import GRUUNet2
        from oracle import model_ref
        model = GRUUNet2(5, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
        model.load_state_dict(model_ref.unflatten_weights(blob))
        return model.eval().to(self.device)

    def cell(self, blob, Cb, x, hx0, mode):
        if mode not in ("module", "module-bf16"):
            return super().cell(blob, Cb, x, hx0, mode)
        model = self.gruunet2(blob)
        model.conv_precision = "bf16" if mode == "module-bf16" else "fp32"
        out, hx = model(self.up(x), self.up(hx0))
        return self.down(out), self.down(hx)

    def momo(self, blob, pads, x, hx0, prev, via="abi"):
        if via == "abi":
            return super().momo(blob, pads, x, hx0, prev)
        from audio_denoising_amd.momo3 import MOMO3
        from oracle import momo_ref
        model = MOMO3(hx0.shape[2], 1, (16, 16, 16), (3, 3, 3), (2, 2, 2), tuple(pads))
        model.load_state_dict(momo_ref.unflatten_weights(blob))
        model.eval().to(self.device)
        out, hx = model(self.up(x), self.up(hx0), prev=None if prev is None else self.up(prev))
        return self.down(out), self.down(hx), self.down(MOMO3.last_frame(self.up(x)))[:, 0, :]

    def process_frame(self, p, frames, hx0):
        """Denoiser.process_frame(return_residual=True); the C ABI where the Denoiser's own plan cannot be built (80 mels at n_fft 512 leave
        filters empty and it passes no pseudo-inverse)"""
        if np.linalg.matrix_rank(mc.hop_fbank(p)) < p.n_mels:
            return super().process_frame(p, frames, hx0)
        from audio_denoising_amd.pipeline import Denoiser
        dn = Denoiser(self.gruunet2(mc.hop_blob()), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=mc.HOP_N_ITER)
        out, hx, resid = dn.process_frame(self.up(frames), self.up(hx0), seed=11, stream_id0=3, return_residual=True)
        assert torch.isfinite(out).all()
        return self.down(resid), self.down(hx)
