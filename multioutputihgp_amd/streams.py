"""Batched, device-resident entry points (include/moihgp.h part 2) over torch tensors.

torch is plumbing here: it owns device memory and streams; all arithmetic is in libmoihgp.so.

Stream layout: SERIES-MAJOR `[L, ld]` (one contiguous row per latent), fp32 or fp64.  The per-tick loop of
the reference callers (`for y in data: gp.step(x, y)`, example.py:40-42; moihgp_online.h:61-70;
moihgp_regression.h:42-50) becomes ONE call over T ticks.

Segment-major streams `[ceil(T / SEG), L, SEG]` (`alloc_stream_tiled`): `project_stream_tiled` -> `LatentBank.filter_tiled` ->
`unproject_stream_tiled` is the same pipeline without a copy between layouts; `filter_outputs` picks one of the two.

Ordering (include/moihgp.h "ordering contract"): `filter`, `grad`, `project_stream`, `unproject_stream` (and the tiled forms) are asynchronous on
the torch stream they are given and read the handle's tables; `LatentBank.update`, `MOIHGP.update` and `set_mixing` first wait
(on the device) for all such work already enqueued through the handle, then rewrite the tables and return when they are
complete -- an update issued behind pipelined sweeps neither overtakes them nor needs a host synchronisation from the caller.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from ._lib import MoihgpError, c_double_p, last_error, load_library

KERNEL_ID = {"Matern32": 0, "Matern52": 1, "Matern52ss": 1}
for _J in (2, 3, 4):          # stacked kernels (include/moihgp.h MOIHGP_STACK): "<base>x<J>", filter mode only
    KERNEL_ID["Matern32x%d" % _J] = 0 | (_J << 4)
    KERNEL_ID["Matern52x%d" % _J] = 1 | (_J << 4)
_DT = {torch.float64: 0, torch.float32: 1}


def _check(rc, lib):
    if rc != 0:
        raise MoihgpError(last_error(lib) or f"libmoihgp call failed (rc={rc})", rc)


def _stream_ptr(stream=None):
    s = torch.cuda.current_stream() if stream is None else stream
    return C.c_void_p(s.cuda_stream)


def padded_len(T: int, dtype) -> int:
    """Row length that satisfies the alignment contract of moihgp_filter_stream (16-byte vectors)."""
    epv = 2 if dtype == torch.float64 else 4
    return (T + epv - 1) // epv * epv


def alloc_stream(L: int, T: int, dtype=torch.float32, device="cuda") -> torch.Tensor:
    """[L, ld] tensor with ld = T rounded up; use `[:, :T]` for the payload."""
    return torch.empty((L, padded_len(T, dtype)), dtype=dtype, device=device)


def seg_ticks(dtype) -> int:
    """Ticks per tile of the segment-major layout: 4 KB of stream (include/moihgp.h moihgp_filter_stream_tiled)."""
    return 512 if dtype == torch.float64 else 1024


def alloc_stream_tiled(L: int, T: int, dtype=torch.float32, device="cuda") -> torch.Tensor:
    """Segment-major stream [ceil(T / SEG), L, SEG]: tile (s, l) holds ticks [s SEG, (s + 1) SEG) of latent l; the last tile is whole."""
    seg = seg_ticks(dtype)
    return torch.empty(((T + seg - 1) // seg, L, seg), dtype=dtype, device=device)


def tile_stream(Ty: torch.Tensor, T: Optional[int] = None, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """Series-major [L, ld] -> segment-major [ceil(T / SEG), L, SEG] (ticks past T become zeros), by the library's copy kernel."""
    lib = load_library()
    L, ld = Ty.shape
    T = ld if T is None else int(T)
    if out is None:
        out = alloc_stream_tiled(L, T, Ty.dtype, Ty.device)
    _check(lib.moihgp_stream_retile(_DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), C.c_void_p(out.data_ptr()), L, T, Ty.stride(0), 1, _stream_ptr(stream)), lib)
    return out


def untile_stream(Tt: torch.Tensor, T: int, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """Segment-major [nseg, L, SEG] -> series-major [L, ld] (the first T ticks of every latent)."""
    lib = load_library()
    L = Tt.shape[1]
    if out is None:
        out = alloc_stream(L, T, Tt.dtype, Tt.device)
    _check(lib.moihgp_stream_retile(_DT[Tt.dtype], C.c_void_p(Tt.data_ptr()), C.c_void_p(out.data_ptr()), L, T, out.stride(0), 0, _stream_ptr(stream)), lib)
    return out


FORECAST_MAX_HORIZONS = 8       # MOIHGP_FORECAST_MAX_HORIZONS
LAGGED_MAX_LAGS = 8             # MOIHGP_LAGGED_MAX_LAGS
INTERP_MAX_POINTS = 8           # MOIHGP_INTERP_MAX_POINTS
_GAINS = {"kalman": 0, "handle": 1}
_GIVEN = {"all": 0, "past": 1}  # MOIHGP_SLOPE_ALL, MOIHGP_SLOPE_PAST


def _int_list(values, noun: str, most: int):
    """(ctypes int array, K) of a forecast's horizons (noun "horizon", at most FORECAST_MAX_HORIZONS) or a fixed-lag smoother's lags ("lag",
    LAGGED_MAX_LAGS), validated as include/moihgp.h states them."""
    try:
        vs = [v for v in values]
    except TypeError:
        raise ValueError(f"{noun}s must be a sequence of 1 .. 8 integers") from None
    if not 1 <= len(vs) <= most:
        raise ValueError(f"the number of {noun}s ({len(vs)}) must be 1 .. {most}")
    for v in vs:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0 or v > (1 << 20):
            raise ValueError(f"{noun} {v!r} must be an integer in 0 .. 2^20")
    return (C.c_int * len(vs))(*[int(v) for v in vs]), len(vs)


def _frac_list(values, most: int = INTERP_MAX_POINTS):
    """(ctypes double array, K) of an off-grid smoother's offsets: 1 .. INTERP_MAX_POINTS finite numbers in [0, 1), validated as include/moihgp.h
    states them."""
    if isinstance(values, (str, bytes)):
        raise ValueError("fracs must be a sequence of 1 .. 8 numbers in [0, 1)")
    try:
        vs = [v for v in values]
    except TypeError:
        raise ValueError("fracs must be a sequence of 1 .. 8 numbers in [0, 1)") from None
    if not 1 <= len(vs) <= most:
        raise ValueError(f"the number of offsets ({len(vs)}) must be 1 .. {most}")
    for v in vs:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not 0 <= v < 1:
            raise ValueError(f"offset {v!r} must be a finite number in [0, 1)")
    return (C.c_double * len(vs))(*[float(v) for v in vs]), len(vs)


def _given_flag(given) -> int:
    """MOIHGP_SLOPE_ALL / _PAST of a slope call's `given`: "all" or "past", else ValueError."""
    if not isinstance(given, str) or given not in _GIVEN:
        raise ValueError(f'given {given!r} must be "all" or "past"')
    return _GIVEN[given]


def _row_stride(name: str, buf: torch.Tensor, T: int, Ty: torch.Tensor, also: str = "") -> int:
    """Row stride a C entry is given for the caller's row buffer `buf` [L, >=T] of the stream Ty, or ValueError (`also`: a further sentence for its text)."""
    L = Ty.shape[0]
    if (not buf.is_cuda or buf.dtype != Ty.dtype or buf.dim() != 2 or buf.stride(1) != 1 or buf.shape[0] != L or buf.shape[1] < T
            or (L > 1 and buf.stride(0) < padded_len(T, Ty.dtype)) or buf.stride(0) % (2 if Ty.dtype == torch.float64 else 4) != 0):
        raise ValueError(f"{name} must be a CUDA tensor [L, >=T] of the stream's dtype, unit stride along time, row stride a multiple of "
                         f"16 bytes and >= T rounded up to it{also}")
    return buf.stride(0) if L > 1 else padded_len(max(T, 1), Ty.dtype)


def _forecast_gains(gains) -> int:
    if gains not in _GAINS:
        raise ValueError('gains must be "kalman" or "handle"')
    return _GAINS[gains]


def _first_origin(t_first, T: int) -> int:
    """t_first of forecast_scores: an integer in 0 .. T, or ValueError."""
    if isinstance(t_first, bool) or not isinstance(t_first, (int, np.integer)) or not 0 <= t_first <= T:
        raise ValueError(f"t_first {t_first!r} must be an integer in 0 .. T ({T})")
    return int(t_first)


def _plane_strides(out: torch.Tensor, K: int, L: int, T: int, dtype, device):
    """(ld_out, plane_stride) of a buffer of K planes [K, L, >=T] of `dtype` on `device`, or ValueError: shape, unit stride along time, row and plane
    strides multiples of 16 bytes, rows >= T rounded up, planes >= L rows."""
    epv = 2 if dtype == torch.float64 else 4
    ok = (out.device == device and out.dtype == dtype and out.dim() == 3 and out.shape[0] == K and out.shape[1] == L and out.shape[2] >= T
          and (out.shape[2] <= 1 or out.stride(2) == 1) and out.data_ptr() % 16 == 0)
    if ok:
        ld_out = out.stride(1) if L > 1 else padded_len(max(T, 1), dtype)
        plane = out.stride(0) if K > 1 else L * ld_out
        ok = ld_out % epv == 0 and ld_out >= padded_len(T, dtype) and plane % epv == 0 and plane >= L * ld_out
    if not ok:
        raise ValueError("out must be a tensor [K, L, >=T] of the stream's dtype and device, 16-byte aligned, unit stride along time, row stride a "
                         "multiple of 16 bytes and >= T rounded up to it, plane stride a multiple of 16 bytes and >= L rows")
    return ld_out, plane


def _plane_out_strides(out: torch.Tensor, K: int, L: int, T: int, Ty: torch.Tensor):
    """(ld_out, plane_stride) of a buffer of K planes [K, L, >=T] (forecast horizons, posterior samples) for the stream Ty, or ValueError:
    dtype, device, shape, unit stride along time, row and plane strides multiples of 16 bytes, rows >= T rounded up, planes >= L rows, and no overlap with Ty."""
    ld_out, plane = _plane_strides(out, K, L, T, Ty.dtype, Ty.device)
    es = Ty.element_size()
    a0, a1 = Ty.data_ptr(), Ty.data_ptr() + L * Ty.stride(0) * es
    b0, b1 = out.data_ptr(), out.data_ptr() + ((K - 1) * plane + L * ld_out) * es
    if T > 0 and a0 < b1 and b0 < a1:
        raise ValueError("out must not overlap the input stream")
    return ld_out, plane


class LatentBank:
    """A shard of independent latent IHGPs (reference include/moihgp/ihgp.h `IHGP<SS>` x L) on one GPU.

    Holds the stationary matrices of `L` latents (computed on device by `IHGP::update`, ihgp.h:117-201)
    and runs the per-latent recursion + NLL over whole streams.
    """

    def __init__(self, dt: float, params_LP, kernel: str = "Matern52ss"):
        self._lib = load_library()
        kid = KERNEL_ID[kernel]
        J = kid >> 4
        self.stacked = J > 0
        self.P = 2 * J + 1 if J else 3
        self.d = (2 if (kid & 15) == 0 else 3) * max(J, 1)
        p = np.ascontiguousarray(np.asarray(params_LP, dtype=np.float64).reshape(-1, self.P))
        self.L = p.shape[0]
        self.kernel = kernel
        self._h = self._lib.moihgp_new_latents(KERNEL_ID[kernel], float(dt), self.L, p.ctypes.data_as(c_double_p))
        if not self._h:
            raise MoihgpError(last_error(self._lib) or "moihgp_new_latents failed")
        self.device = torch.device("cuda", torch.cuda.current_device())

    @classmethod
    def from_handle(cls, gp):
        """View the latents of a full `MOIHGP` object (pywrapper.MOIHGP) without copying."""
        self = cls.__new__(cls)
        self._lib = load_library()
        self._h = gp.handle
        self._owner = gp
        self.L = gp.num_latent
        self.d = gp.igp_dim
        self.P = gp.num_igp_param
        self.kernel = None
        self.stacked = gp.igp_dim > 3
        self.device = torch.device("cuda", torch.cuda.current_device())
        return self

    def __del__(self):
        try:
            if getattr(self, "_owner", None) is None and self._h:
                self._lib.moihgp_del(self._h)
                self._h = None
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        """Per-handle tuning / test hooks (include/moihgp.h moihgp_set_option): "filter_split" (0 automatic, 1 off, n slices),
        "filter_maxlinks", "filter_variant" (tuning builds only), "smoother_path", "forecast_path", "sample_path", "lagged_path", "interp_path" (-1 automatic, 0 scan kernels, 1 serial fp64)."""
        _check(self._lib.moihgp_set_option(self._h, name.encode(), int(value)), self._lib)

    def update(self, params_LP):
        p = np.ascontiguousarray(np.asarray(params_LP, dtype=np.float64).reshape(self.L, self.P))
        _check(self._lib.moihgp_update_latents(self._h, p.ctypes.data_as(c_double_p)), self._lib)

    def latent(self, l: int) -> dict:
        d, P = self.d, self.P
        out = dict(A=np.zeros((d, d)), K=np.zeros(d), S=np.zeros(1), HA=np.zeros(d), AKHA=np.zeros((d, d)),
                   dA=np.zeros((P, d, d)), dS=np.zeros(P), dK=np.zeros((P, d)), dAKHA=np.zeros((P, d, d)), HdA=np.zeros((P, d)))
        iters = (C.c_int * (1 + P))()
        ptrs = [out[k].ctypes.data_as(c_double_p) if k in out else None for k in ("A", "K", "S", "HA", "AKHA", "dA", "dS", "dK", "dAKHA", "HdA")]
        _check(self._lib.moihgp_get_latent(self._h, l, *ptrs, iters), self._lib)
        out["S"] = float(out["S"][0])
        out["iters"] = list(iters)
        return out

    def profile_enable(self, max_launches: int, stride: int = 1):
        """Attach HIP event pairs to filter dispatches (kernel-exact timing): to every `stride`-th one, `max_launches` pairs
        at most.  A pair costs a few microseconds of launch overlap, so a timed loop samples rather than brackets every pass."""
        _check(self._lib.moihgp_profile_enable(self._h, int(max_launches)), self._lib)
        _check(self._lib.moihgp_profile_stride(self._h, int(stride)), self._lib)
        self._prof_cap = int(max_launches)

    def profile_read(self):
        """Per-launch kernel durations (ms) of the filter dispatches since the last read."""
        n = getattr(self, "_prof_cap", 0)
        buf = (C.c_float * max(n, 1))()
        cnt = self._lib.moihgp_profile_read(self._h, buf, n)
        return [float(buf[i]) for i in range(max(cnt, 0))]

    # ---------------------------------------------------------------------------------------
    def _check_stream(self, Ty: torch.Tensor, T: Optional[int]):
        if not Ty.is_cuda or Ty.dtype not in _DT or Ty.dim() != 2 or Ty.shape[0] != self.L or Ty.stride(1) != 1:
            raise ValueError("Ty must be a CUDA tensor [L, ld] (float32/float64) with unit stride along time")
        T = Ty.shape[1] if T is None else int(T)
        if T < 0 or T > Ty.shape[1]:
            raise ValueError("T exceeds the stream tensor")
        return T, Ty.stride(0)

    @staticmethod
    def _like_stream(Ty: torch.Tensor) -> torch.Tensor:
        """Output stream with the SAME row stride as Ty (Ty may be a column slice of a wider slab)."""
        buf = torch.empty((Ty.shape[0], Ty.stride(0)), dtype=Ty.dtype, device=Ty.device)
        return buf[:, :Ty.shape[1]]

    def filter(self, Ty: torch.Tensor, T: Optional[int] = None, x: Optional[torch.Tensor] = None,
               want_yhat: bool = True, want_nll: bool = True, yhat: Optional[torch.Tensor] = None,
               nll: Optional[torch.Tensor] = None, stream=None, x_start: Optional[torch.Tensor] = None,
               nll_total: Optional[torch.Tensor] = None):
        """One sweep of ihgp.h:81-93 (+ :204-209 on the pre-step state) over T ticks for every latent.

        Returns (yhat [L, ld] or None, x [L, d] final state, nll [L] float64 or None).  Asynchronous on
        the current torch stream.  `x` (initial state) is updated IN PLACE if given.  With `x_start` the sweep starts from
        that state instead (left untouched) and `x` only receives the final state: no reset between repeated sweeps.
        `nll_total` (a 1-element float64 CUDA tensor) receives the sum of the per-latent NLLs (one-wavefront kernel queued behind the sweep)."""
        T, ld = self._check_stream(Ty, T)
        if x is None:
            x = torch.zeros((self.L, self.d), dtype=Ty.dtype, device=Ty.device)
        if want_yhat:
            if yhat is None:
                yhat = self._like_stream(Ty)
            else:
                _row_stride("yhat", yhat, T, Ty, " (it need not equal the stream's: moihgp_filter_stream_v2 takes both)")
        if x.dtype != Ty.dtype or not x.is_contiguous() or tuple(x.shape) != (self.L, self.d):
            raise ValueError("x must be a contiguous [L, d] tensor of the stream dtype")
        if want_nll and nll is None:
            nll = torch.empty((self.L,), dtype=torch.float64, device=Ty.device)
        if x_start is not None and (x_start.dtype != Ty.dtype or not x_start.is_contiguous() or tuple(x_start.shape) != (self.L, self.d)):
            raise ValueError("x_start must be a contiguous [L, d] tensor of the stream dtype")
        rc = self._lib.moihgp_filter_stream_v2(
            self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld, C.c_void_p((x if x_start is None else x_start).data_ptr()),
            C.c_void_p(x.data_ptr()),
            C.c_void_p(yhat.data_ptr()) if want_yhat else None, ((yhat.stride(0) if self.L > 1 else padded_len(T, Ty.dtype)) if want_yhat else 0),
            C.c_void_p(nll.data_ptr()) if want_nll else None,
            C.c_void_p(nll_total.data_ptr()) if (nll_total is not None and want_nll) else None, _stream_ptr(stream))
        _check(rc, self._lib)
        return (yhat if want_yhat else None), x, (nll if want_nll else None)

    def filter_tiled(self, Tt: torch.Tensor, T: int, x: Optional[torch.Tensor] = None, want_yhat: bool = True, want_nll: bool = True,
                     yhat: Optional[torch.Tensor] = None, nll: Optional[torch.Tensor] = None, stream=None, x_start: Optional[torch.Tensor] = None,
                     nll_total: Optional[torch.Tensor] = None):
        """`filter` over a SEGMENT-MAJOR stream [ceil(T / SEG), L, SEG] (alloc_stream_tiled / tile_stream): same arithmetic, same results bit for
        bit; the chip reads and writes one contiguous front instead of L row streams (moihgp_filter_stream_tiled).  yhat comes back in the
        same layout.  The reference's own models only (d = 2, 3)."""
        seg = seg_ticks(Tt.dtype)
        nseg = (int(T) + seg - 1) // seg
        if not Tt.is_cuda or Tt.dtype not in _DT or not Tt.is_contiguous() or tuple(Tt.shape) != (nseg, self.L, seg):
            raise ValueError(f"Tt must be a contiguous CUDA tensor [ceil(T / {seg}) = {nseg}, L = {self.L}, {seg}]")
        if x is None:
            x = torch.zeros((self.L, self.d), dtype=Tt.dtype, device=Tt.device)
        if x.dtype != Tt.dtype or not x.is_contiguous() or tuple(x.shape) != (self.L, self.d):
            raise ValueError("x must be a contiguous [L, d] tensor of the stream dtype")
        if x_start is not None and (x_start.dtype != Tt.dtype or not x_start.is_contiguous() or tuple(x_start.shape) != (self.L, self.d)):
            raise ValueError("x_start must be a contiguous [L, d] tensor of the stream dtype")
        if want_yhat:
            if yhat is None:
                yhat = torch.empty_like(Tt)
            elif not yhat.is_cuda or yhat.dtype != Tt.dtype or not yhat.is_contiguous() or tuple(yhat.shape) != tuple(Tt.shape):
                raise ValueError("yhat must be a contiguous CUDA tensor shaped like the stream")
        if want_nll and nll is None:
            nll = torch.empty((self.L,), dtype=torch.float64, device=Tt.device)
        rc = self._lib.moihgp_filter_stream_tiled(
            self._h, _DT[Tt.dtype], C.c_void_p(Tt.data_ptr()), int(T), C.c_void_p((x if x_start is None else x_start).data_ptr()), C.c_void_p(x.data_ptr()),
            C.c_void_p(yhat.data_ptr()) if want_yhat else None, C.c_void_p(nll.data_ptr()) if want_nll else None,
            C.c_void_p(nll_total.data_ptr()) if (nll_total is not None and want_nll) else None, _stream_ptr(stream))
        _check(rc, self._lib)
        return (yhat if want_yhat else None), x, (nll if want_nll else None)

    def grad(self, Ty: torch.Tensor, T: Optional[int] = None, x: Optional[torch.Tensor] = None,
             dx: Optional[torch.Tensor] = None, want_yhat: bool = False, stream=None):
        """Sweep with sensitivities (ihgp.h:37-57) and the per-latent NLL gradient (ihgp.h:212-222).

        Returns dict(yhat, x, dx, nll [L], grad [L, P])."""
        T, ld = self._check_stream(Ty, T)
        if x is None:
            x = torch.zeros((self.L, self.d), dtype=Ty.dtype, device=Ty.device)
        if dx is None:
            dx = torch.zeros((self.L, self.P, self.d), dtype=Ty.dtype, device=Ty.device)
        if x.dtype != Ty.dtype or dx.dtype != Ty.dtype or not x.is_contiguous() or not dx.is_contiguous():
            raise ValueError("x / dx must be contiguous tensors of the stream dtype")
        yhat = self._like_stream(Ty) if want_yhat else None
        nll = torch.empty((self.L,), dtype=torch.float64, device=Ty.device)
        grad = torch.empty((self.L, self.P), dtype=torch.float64, device=Ty.device)
        rc = self._lib.moihgp_grad_stream(
            self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld, C.c_void_p(x.data_ptr()), C.c_void_p(dx.data_ptr()),
            C.c_void_p(yhat.data_ptr()) if want_yhat else None, C.c_void_p(nll.data_ptr()), C.c_void_p(grad.data_ptr()),
            _stream_ptr(stream))
        _check(rc, self._lib)
        return dict(yhat=yhat, x=x, dx=dx, nll=nll, grad=grad)

    def _start_state(self, Ty: torch.Tensor, x: Optional[torch.Tensor], x_start: Optional[torch.Tensor]):
        """(x, start) of smooth / forecast: `x` [L, d] receives the end state (zeros if not given), the sweep starts from `x_start` if given, else from `x`."""
        if x is None:
            x = torch.zeros((self.L, self.d), dtype=Ty.dtype, device=Ty.device)
        for name, t in (("x", x), ("x_start", x_start)):
            if t is not None and (t.dtype != Ty.dtype or not t.is_contiguous() or tuple(t.shape) != (self.L, self.d)):
                raise ValueError(f"{name} must be a contiguous [L, d] tensor of the stream dtype")
        return x, (x if x_start is None else x_start)

    def _ysmooth_buffer(self, Ty: torch.Tensor, T: int, ysmooth: Optional[torch.Tensor]):
        """(ysmooth, ld_out) of smooth / sample: the caller's buffer, checked, or a fresh one."""
        if ysmooth is None:
            ysmooth = alloc_stream(self.L, max(T, 1), Ty.dtype, Ty.device)[:, :T]
        return ysmooth, _row_stride("ysmooth", ysmooth, T, Ty)

    def _plane_and_row_buffers(self, Ty: torch.Tensor, T: int, K: int, out: Optional[torch.Tensor], rows: Optional[torch.Tensor]):
        """(out, ld_out, plane, rows, hand_over) of sample / lagged, which write K planes `out` [K, L, >=T] and a row buffer `rows` [L, >=T] (ysmooth,
        ypred): the caller's buffers, checked, or fresh ones.  One row stride serves both buffers in the C entry: rows without a buffer of their own
        take the planes' stride, and a caller's `rows` of another stride is replaced by a buffer of that stride for the call; hand_over(stream),
        called behind the sweep, copies it into the caller's tensor and returns the tensor to hand back."""
        if out is None:
            rows, ld_out = self._ysmooth_buffer(Ty, T, rows)
            out = torch.empty((K, self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :, :T]
        ld_out, plane = _plane_out_strides(out, K, self.L, T, Ty)
        mine = rows
        if rows is None or (self._ysmooth_buffer(Ty, T, rows)[1] != ld_out and self.L > 1):
            mine = torch.empty((self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :T]

        def hand_over(stream):
            if rows is None or mine is rows:
                return mine
            with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
                rows[:, :T].copy_(mine)
            return rows
        return out, ld_out, plane, mine, hand_over

    def _refuse_stacked(self, who: str):
        if self.stacked:
            raise MoihgpError(f"{who}: stacked models are not supported (Matern-3/2 and -5/2 only)", 3)

    def smooth(self, Ty: torch.Tensor, T: Optional[int] = None, x: Optional[torch.Tensor] = None, x_start: Optional[torch.Tensor] = None,
               ysmooth: Optional[torch.Tensor] = None, stream=None):
        """Steady-state RTS smoothing of T ticks for every latent (include/moihgp.h moihgp_smooth_stream): the posterior mean at every tick
        given the whole stream, with the Kalman DARE's gains (not the learners' literal ones).

        Returns (ysmooth [L, >=T], x [L, d] end state (filtered = smoothed), status [L] int32: 0 ok, 1 DARE not converged (row NaN)).
        Asynchronous on the current torch stream.  The sweep starts from `x_start` if given, else from `x`, else from zeros; `x` receives the
        end state in place.  `ysmooth` (optional) must not overlap Ty; its row stride may differ from the stream's."""
        T, ld = self._check_stream(Ty, T)
        self._refuse_stacked("smooth")
        x, start = self._start_state(Ty, x, x_start)
        ysmooth, ld_out = self._ysmooth_buffer(Ty, T, ysmooth)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_smooth_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                            C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()),
                                            C.c_void_p(ysmooth.data_ptr()), ld_out, C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return ysmooth, x, status

    def smooth_exact(self, Ty: torch.Tensor, T: Optional[int] = None, x: Optional[torch.Tensor] = None, ysmooth: Optional[torch.Tensor] = None,
                     var: Optional[torch.Tensor] = None, want_var: bool = True, stream=None):
        """Exact-edge smoothing of T ticks for every latent (include/moihgp.h moihgp_smooth_stream_exact): `smooth` from the prior (a zero start
        state), corrected at the head of the stream for the model's own prior on the first state, with the posterior variance of the latent
        function at every tick.  For a gap-free stream this is the GP posterior at every tick, for any T >= 1.

        Returns (ysmooth [L, >=T], var [L, >=T] or None, x [L, d] end state, status [L] int32: 0 ok, 1 DARE not converged (rows NaN), 3 the
        latent's edges overlap in a stream longer than 4096 ticks, 4 its edge tables failed (3, 4: the row and x are `smooth`'s, var is
        var_smoothed)).  Asynchronous on the current torch stream, but for the first call after an update, which reads the edge lengths back.
        `x` receives the end state (it is not a start state).  `ysmooth` and `var` (optional) must not overlap Ty or each other and share one row
        stride, which may differ from the stream's; `want_var=False` (with no `var`) writes no variance."""
        T, ld = self._check_stream(Ty, T)
        self._refuse_stacked("smooth_exact")
        x, _ = self._start_state(Ty, x, None)
        if ysmooth is None and var is not None:
            ld_out = _row_stride("var", var, T, Ty)
            ysmooth = torch.empty((self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :T]
        ysmooth, ld_out = self._ysmooth_buffer(Ty, T, ysmooth)
        if var is None and want_var:
            var = torch.empty((self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :T]
        if var is not None and _row_stride("var", var, T, Ty) != ld_out:
            raise ValueError("var and ysmooth must have the same row stride")
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_smooth_stream_exact(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld, C.c_void_p(x.data_ptr()),
                                                  C.c_void_p(ysmooth.data_ptr()), C.c_void_p(var.data_ptr()) if var is not None else None, ld_out,
                                                  C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return ysmooth, var, x, status

    def edge_lengths(self):
        """(head [L], tail [L]) of every latent (moihgp_edge_lengths), int numpy arrays: `smooth_exact` touches the ticks before `head` and the
        last `tail` ticks of a row; 2^20 means "never reached"."""
        self._refuse_stacked("edge_lengths")
        head, tail = np.zeros(self.L, dtype=np.int32), np.zeros(self.L, dtype=np.int32)
        ip = C.POINTER(C.c_int)
        _check(self._lib.moihgp_edge_lengths(self._h, head.ctypes.data_as(ip), tail.ctypes.data_as(ip)), self._lib)
        return head, tail

    def posterior(self, Ty: torch.Tensor, T: Optional[int] = None, x: Optional[torch.Tensor] = None, mean: Optional[torch.Tensor] = None,
                  var: Optional[torch.Tensor] = None, want_var: bool = True, want_nll: bool = True, want_cov: bool = False, stream=None):
        """Exact smoothing of T ticks across missing ticks for every latent (include/moihgp.h moihgp_posterior_stream): the time-varying Kalman
        filter from the model's own prior and the RTS backward pass, with no update at a NaN tick.  For any pattern of missing ticks this is the
        GP posterior at every tick; no steady-state gain and no DARE is involved.  Serial in time: 4 to 5 us per tick at 16 to 4096
        latents, far above `smooth_exact`.

        Returns dict(mean [L, >=T], var [L, >=T] or None (the latent function's, no noise), x [L, d] the filtered end state, P_end [L, d, d] fp64 or
        None (its covariance; `want_cov`), nll [L] fp64 or None (the exact -log marginal likelihood of the observed ticks; `want_nll`), status [L]
        int32: 0 ok, 5 the recursion broke down (the latent's outputs are NaN)).  Asynchronous on the current torch stream.  `x` receives the
        end state (it is not a start state: the start is the prior).  `mean` and `var` (optional) must not overlap Ty or each other and share one
        row stride, which may differ from the stream's; `want_var=False` (with no `var`) writes no variance."""
        T, ld = self._check_stream(Ty, T)
        self._refuse_stacked("posterior")
        x, _ = self._start_state(Ty, x, None)
        if mean is None and var is not None:
            ld_out = _row_stride("var", var, T, Ty)
            mean = torch.empty((self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :T]
        if mean is None:
            mean = alloc_stream(self.L, max(T, 1), Ty.dtype, Ty.device)[:, :T]
        ld_out = _row_stride("mean", mean, T, Ty)
        if var is None and want_var:
            var = torch.empty((self.L, ld_out), dtype=Ty.dtype, device=Ty.device)[:, :T]
        if var is not None and _row_stride("var", var, T, Ty) != ld_out:
            raise ValueError("var and mean must have the same row stride")
        P_end = torch.empty((self.L, self.d, self.d), dtype=torch.float64, device=Ty.device) if want_cov else None
        nll = torch.empty((self.L,), dtype=torch.float64, device=Ty.device) if want_nll else None
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        rc = self._lib.moihgp_posterior_stream(self._h, _DT[Ty.dtype], ptr(Ty), T, ld, ptr(x), ptr(P_end), ptr(mean), ptr(var), ld_out, ptr(nll),
                                               ptr(status), _stream_ptr(stream))
        _check(rc, self._lib)
        return dict(mean=mean, var=var, x=x, P_end=P_end, nll=nll, status=status)

    def smoother(self, l: int) -> dict:
        """The smoother's stationary quantities of latent l (moihgp_get_smoother): P (Kalman DARE), K, G, Ps, var_filtered, var_smoothed."""
        d = self.d
        out = dict(P=np.zeros((d, d)), K=np.zeros(d), G=np.zeros((d, d)), Ps=np.zeros((d, d)), var_filtered=np.zeros(1), var_smoothed=np.zeros(1))
        ptrs = [out[k].ctypes.data_as(c_double_p) for k in ("P", "K", "G", "Ps", "var_filtered", "var_smoothed")]
        _check(self._lib.moihgp_get_smoother(self._h, int(l), *ptrs), self._lib)
        out["var_filtered"] = float(out["var_filtered"][0])
        out["var_smoothed"] = float(out["var_smoothed"][0])
        return out

    def latent_variances(self):
        """(var_filtered [L], var_smoothed [L]) of every latent (moihgp_latent_variances), fp64 numpy arrays."""
        vf, vs = np.zeros(self.L), np.zeros(self.L)
        _check(self._lib.moihgp_latent_variances(self._h, vf.ctypes.data_as(c_double_p), vs.ctypes.data_as(c_double_p)), self._lib)
        return vf, vs

    def sample(self, Ty: torch.Tensor, nsamples: int, seed: int = 0, sample0: int = 0, latent0: int = 0, T: Optional[int] = None,
               x: Optional[torch.Tensor] = None, x_start: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
               ysmooth: Optional[torch.Tensor] = None, stream=None):
        """Seeded steady-state posterior samples of T ticks for every latent (include/moihgp.h moihgp_sample_stream): samples[s, l] is the smoothed
        mean of latent l plus a draw of the stationary deviation process with the steady-state posterior's covariance across time (exact in the
        interior of a long gap-free stream, under-dispersed near the ends and missing ticks, as var_smoothed).  The noise is Philox4x32-10 keyed by
        `seed` (64 bits) and counted by (tick, latent0 + l, sample0 + s): calls for ranges of samples or latents reproduce one large call bit for bit.

        Returns (samples [S, L, >=T], ysmooth [L, >=T], x [L, d] end state, status [L] int32: 0 ok, 1 Kalman DARE not converged (all NaN),
        2 realization not accepted (sample rows NaN, ysmooth as smooth())).  Asynchronous on the current torch stream.  `x`, `x_start`, `ysmooth` as
        smooth(); `out` (optional) [S, L, >=T] as forecast()'s; `out` and `ysmooth` must not overlap Ty or each other."""
        T, ld = self._check_stream(Ty, T)
        S = int(nsamples)
        if not 1 <= S <= 65535:
            raise ValueError("nsamples must be 1 .. 65535")
        seed, sample0, latent0 = int(seed), int(sample0), int(latent0)
        if not (0 <= seed < 1 << 64 and 0 <= sample0 < 1 << 32 and 0 <= latent0 < 1 << 32):
            raise ValueError("seed must be in 0 .. 2^64 - 1, sample0 and latent0 in 0 .. 2^32 - 1")
        self._refuse_stacked("sample")
        x, start = self._start_state(Ty, x, x_start)
        out, ld_out, plane, ysmooth, hand_over = self._plane_and_row_buffers(Ty, T, S, out, ysmooth)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_sample_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                            C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), S, seed, sample0, latent0,
                                            C.c_void_p(ysmooth.data_ptr()), ld_out, C.c_void_p(out.data_ptr()), plane,
                                            C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, hand_over(stream), x, status

    def sampler(self, l: int) -> dict:
        """The sampler's realization of latent l (moihgp_get_sampler): B, sigma2, Sigma, Lc, acov_err, status."""
        d = self.d
        out = dict(B=np.zeros(d), sigma2=np.zeros(1), Sigma=np.zeros((d, d)), Lc=np.zeros((d, d)), acov_err=np.zeros(1))
        st = C.c_int(0)
        ptrs = [out[k].ctypes.data_as(c_double_p) for k in ("B", "sigma2", "Sigma", "Lc", "acov_err")]
        _check(self._lib.moihgp_get_sampler(self._h, int(l), *ptrs, C.byref(st)), self._lib)
        out["sigma2"] = float(out["sigma2"][0])
        out["acov_err"] = float(out["acov_err"][0])
        out["status"] = int(st.value)
        return out

    def forecast(self, Ty: torch.Tensor, horizons, T: Optional[int] = None, x: Optional[torch.Tensor] = None, x_start: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, gains: str = "kalman", stream=None):
        """Forecasts at every tick of T ticks for every latent (include/moihgp.h moihgp_forecast_stream): fc[k, l, t] is the mean of latent l at tick
        t + horizons[k] given the ticks <= t, stored at the tick the forecast is made at (missing ticks included).  horizons: 1 .. 8 ints in
        0 .. 2^20, in any order.  gains "kalman" (default): the smoother's Kalman-form gains, the GP predictive mean in the interior of a stream, with
        forecast_variances() as its variance; "handle": the handle's own gains, i.e. filter()'s estimator followed by h prediction-only steps.

        Returns (fc [K, L, >=T], x [L, d] end state, status [L] int32: 0 ok, 1 Kalman DARE not converged (rows NaN; always 0 with "handle")).
        Asynchronous on the current torch stream.  The sweep starts from `x_start` if given, else from `x`, else from zeros; `x` receives the end
        state in place.  `out` (optional) [K, L, >=T] must not overlap Ty; row and plane strides multiples of 16 bytes."""
        T, ld = self._check_stream(Ty, T)
        hz, K = _int_list(horizons, "horizon", FORECAST_MAX_HORIZONS)
        g = _forecast_gains(gains)
        self._refuse_stacked("forecast")
        x, start = self._start_state(Ty, x, x_start)
        if out is None:
            out = torch.empty((K, self.L, padded_len(max(T, 1), Ty.dtype)), dtype=Ty.dtype, device=Ty.device)[:, :, :T]
        ld_out, plane = _plane_out_strides(out, K, self.L, T, Ty)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_forecast_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                              C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), hz, K,
                                              C.c_void_p(out.data_ptr()), ld_out, plane, g, C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, x, status

    def forecast_scores(self, Ty: torch.Tensor, horizons, T: Optional[int] = None, t_first: int = 0, x: Optional[torch.Tensor] = None,
                        x_start: Optional[torch.Tensor] = None, gains: str = "kalman", stream=None) -> dict:
        """Backtest errors of forecast()'s forecasts on the stream itself (include/moihgp.h moihgp_forecast_scores), without writing a plane: for
        every horizon k and latent l, over the origins t_first <= t < T whose target tick t + horizons[k] lies inside the stream and is observed,
        e = Ty[l, t + h] - fc[k, l, t]; n counts them, sum_err and sum_sq add e and e^2 in fp64 in a fixed order (two equal calls give equal bits).
        The origin tick itself may be missing.  `t_first` skips the start-up transient of a zero start state.  h = 0 scores the in-sample residual
        against the filtered mean, which is not a prediction error.  horizons and gains as forecast().

        Returns dict(n [K, L] int64, sum_err, sum_sq [K, L] fp64, pvar [K, L] fp64 -- the predictive variance of an observation,
        forecast_variances() + noise, for h >= 1 -- or None with gains "handle", x [L, d] end state, status [L] int32, horizons: the list).  A
        latent whose Kalman DARE did not converge has status 1, n = 0 and NaN elsewhere.  Asynchronous on the current torch stream; `x`, `x_start`
        as forecast().  score_summary() turns the sums into mse, bias, smse and mlpd."""
        T, ld = self._check_stream(Ty, T)
        hz, K = _int_list(horizons, "horizon", FORECAST_MAX_HORIZONS)
        g = _forecast_gains(gains)
        t_first = _first_origin(t_first, T)
        self._refuse_stacked("forecast_scores")
        x, start = self._start_state(Ty, x, x_start)
        n = torch.empty((K, self.L), dtype=torch.int64, device=Ty.device)
        sum_err = torch.empty((K, self.L), dtype=torch.float64, device=Ty.device)
        sum_sq = torch.empty_like(sum_err)
        pvar = torch.empty_like(sum_err) if g == 0 else None
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_forecast_scores(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                              C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), hz, K, t_first, g,
                                              C.c_void_p(n.data_ptr()), C.c_void_p(sum_err.data_ptr()), C.c_void_p(sum_sq.data_ptr()),
                                              C.c_void_p(pvar.data_ptr()) if pvar is not None else None,
                                              C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return dict(n=n, sum_err=sum_err, sum_sq=sum_sq, pvar=pvar, x=x, status=status, horizons=[int(h) for h in hz])

    def lagged(self, Ty: torch.Tensor, lags, T: Optional[int] = None, x: Optional[torch.Tensor] = None, x_start: Optional[torch.Tensor] = None,
               state_at: Optional[int] = None, out: Optional[torch.Tensor] = None, ypred: Optional[torch.Tensor] = None, stream=None):
        """Fixed-lag smoothing of T ticks for every latent (include/moihgp.h moihgp_lagged_stream): lag[k, l, t] is the mean of latent l at tick t
        given the ticks <= min(t + lags[k], T - 1), stored at the tick it estimates, with the smoother's steady-state gains.  lags: 1 .. 8 ints in
        0 .. 2^20, in any order; lag 0 is forecast([0]) (the filtered mean), a lag >= T is smooth(); lagged_variances() gives the variances.

        Returns (lag [K, L, >=T], ypred [L, >=T] the one-step predicted means, x [L, d], status [L] int32: 0 ok, 1 Kalman DARE not converged
        (rows, ypred row and x NaN)).  Asynchronous on the current torch stream.  The sweep starts from `x_start` if given, else from `x`, else from
        zeros; `x` receives in place the filtered state after tick `state_at` - 1 (default T: the end state; 0: the start state).  A stream that
        arrives in slabs: call on slab [t0, t1) plus max(lags) ticks of lookahead with `x_start` the carried state and `state_at` = t1 - t0, keep the
        first t1 - t0 ticks of every plane and carry `x`.  `out` (optional) [K, L, >=T] as forecast()'s, `ypred` (optional) as smooth()'s
        `ysmooth`; `out`, `ypred` and Ty must not overlap each other."""
        T, ld = self._check_stream(Ty, T)
        lg, K = _int_list(lags, "lag", LAGGED_MAX_LAGS)
        state_at = T if state_at is None else state_at
        if isinstance(state_at, bool) or not isinstance(state_at, (int, np.integer)) or not 0 <= state_at <= T:
            raise ValueError(f"state_at {state_at!r} must be an integer in 0 .. T")
        self._refuse_stacked("lagged")
        x, start = self._start_state(Ty, x, x_start)
        out, ld_out, plane, ypred, hand_over = self._plane_and_row_buffers(Ty, T, K, out, ypred)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_lagged_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                            C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), int(state_at), lg, K,
                                            C.c_void_p(ypred.data_ptr()), C.c_void_p(out.data_ptr()), ld_out, plane,
                                            C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, hand_over(stream), x, status

    def lagged_variances(self, lags) -> np.ndarray:
        """var [K, L] (moihgp_lagged_variances), fp64 numpy: the steady-state variance of the latent function at tick t given the ticks <= t + lag
        (add the noise parameter for an observation): var_filtered at lag 0, falling to var_smoothed; NaN for a latent whose Kalman DARE did not
        converge."""
        lg, K = _int_list(lags, "lag", LAGGED_MAX_LAGS)
        var = np.zeros((K, self.L))
        _check(self._lib.moihgp_lagged_variances(self._h, lg, K, var.ctypes.data_as(c_double_p)), self._lib)
        return var

    def interpolate(self, Ty: torch.Tensor, fracs, T: Optional[int] = None, x: Optional[torch.Tensor] = None, x_start: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, ysmooth: Optional[torch.Tensor] = None, stream=None):
        """Off-grid smoothing of T ticks for every latent (include/moihgp.h moihgp_interp_stream): fine[k, l, t] is the mean of latent l at time
        (t + fracs[k]) dt given the whole stream, with the smoother's steady-state gains.  fracs: 1 .. 8 finite numbers in [0, 1), in any order;
        offset 0 is smooth(), and the last column of a plane is the forecast fracs[k] dt past the end; interp_variances() gives the variances.

        Returns (fine [K, L, >=T], ysmooth [L, >=T] the smoothed means on the grid, x [L, d] end state, status [L] int32: 0 ok, 1 Kalman DARE not
        converged (rows, ysmooth row and x NaN)).  Asynchronous on the current torch stream.  `x`, `x_start` as smooth(); `out` (optional)
        [K, L, >=T] as forecast()'s, `ysmooth` (optional) as smooth()'s; `out`, `ysmooth` and Ty must not overlap each other."""
        T, ld = self._check_stream(Ty, T)
        fr, K = _frac_list(fracs)
        self._refuse_stacked("interpolate")
        x, start = self._start_state(Ty, x, x_start)
        out, ld_out, plane, ysmooth, hand_over = self._plane_and_row_buffers(Ty, T, K, out, ysmooth)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_interp_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                            C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), fr, K,
                                            C.c_void_p(ysmooth.data_ptr()), C.c_void_p(out.data_ptr()), ld_out, plane,
                                            C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, hand_over(stream), x, status

    def interp_variances(self, fracs) -> np.ndarray:
        """var [K, L] (moihgp_interp_variances), fp64 numpy: the steady-state variance of the latent function at time (t + frac) dt given the whole
        stream (add the noise parameter for an observation): var_smoothed at offset 0, larger between the ticks; NaN for a latent whose Kalman DARE
        did not converge."""
        fr, K = _frac_list(fracs)
        var = np.zeros((K, self.L))
        _check(self._lib.moihgp_interp_variances(self._h, fr, K, var.ctypes.data_as(c_double_p)), self._lib)
        return var

    def slope(self, Ty: torch.Tensor, fracs=(0.0,), given: str = "all", T: Optional[int] = None, x: Optional[torch.Tensor] = None,
              x_start: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, ysmooth: Optional[torch.Tensor] = None, stream=None):
        """Rate of change of every latent over T ticks (include/moihgp.h moihgp_slope_stream): slope[k, l, t] is the derivative with respect to time
        (the unit of dt, not ticks) of the posterior mean of latent l at time (t + fracs[k]) dt -- given the whole stream (given = "all": the
        derivative of interpolate()'s planes) or given the ticks up to t (given = "past": the slope of the forecast fracs[k] dt ahead of tick t, at
        offset 0 the real-time estimate).  fracs as interpolate()'s; slope_variances() gives the variances.

        Returns (slope [K, L, >=T], ysmooth [L, >=T] the smoothed means on the grid -- None with "past", which runs the forward sweep alone and uses
        the buffer as scratch --, x [L, d] end state, status [L] int32: 0 ok, 1 Kalman DARE not converged (rows and x NaN)).  Asynchronous on the
        current torch stream.  `x`, `x_start`, `out`, `ysmooth` as interpolate()'s; the option "interp_path" governs the route."""
        T, ld = self._check_stream(Ty, T)
        fr, K = _frac_list(fracs)
        flag = _given_flag(given)
        self._refuse_stacked("slope")
        x, start = self._start_state(Ty, x, x_start)
        out, ld_out, plane, ysmooth, hand_over = self._plane_and_row_buffers(Ty, T, K, out, ysmooth)
        status = torch.empty((self.L,), dtype=torch.int32, device=Ty.device)
        rc = self._lib.moihgp_slope_stream(self._h, _DT[Ty.dtype], C.c_void_p(Ty.data_ptr()), T, ld,
                                           C.c_void_p(start.data_ptr()), C.c_void_p(x.data_ptr()), fr, K, flag,
                                           C.c_void_p(ysmooth.data_ptr()), C.c_void_p(out.data_ptr()), ld_out, plane,
                                           C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, (hand_over(stream) if given == "all" else None), x, status

    def slope_variances(self, fracs=(0.0,), given: str = "all") -> np.ndarray:
        """var [K, L] (moihgp_slope_variances), fp64 numpy: the steady-state posterior variance of the latent function's time derivative at time
        (t + frac) dt given the whole stream ("all") or the ticks up to t ("past"); NaN for a latent whose Kalman DARE did not converge."""
        fr, K = _frac_list(fracs)
        var = np.zeros((K, self.L))
        _check(self._lib.moihgp_slope_variances(self._h, fr, K, _given_flag(given), var.ctypes.data_as(c_double_p)), self._lib)
        return var

    def forecast_tail(self, x: torch.Tensor, n: int, stream=None) -> torch.Tensor:
        """tail[l, j] = H A^(j+1) x_l, 0 <= j < n (moihgp_forecast_tail): the forecast beyond the end of a stream from its end state x [L, d]."""
        n = int(n)
        if n < 0 or n > (1 << 20):
            raise ValueError("n must be 0 .. 2^20")
        if x.dtype not in _DT or not x.is_contiguous() or tuple(x.shape) != (self.L, self.d):
            raise ValueError("x must be a contiguous [L, d] tensor (float32/float64)")
        self._refuse_stacked("forecast")
        tail = alloc_stream(self.L, max(n, 1), x.dtype, x.device)
        _check(self._lib.moihgp_forecast_tail(self._h, _DT[x.dtype], C.c_void_p(x.data_ptr()), n, C.c_void_p(tail.data_ptr()), tail.stride(0),
                                              _stream_ptr(stream)), self._lib)
        return tail[:, :n]

    def forecast_variances(self, horizons) -> np.ndarray:
        """var [K, L] (moihgp_forecast_variances), fp64 numpy: the steady-state variance of the latent function at t + h given the ticks <= t, which
        belongs to the "kalman" gains (add the noise parameter for an observation); NaN for a latent whose Kalman DARE did not converge."""
        hz, K = _int_list(horizons, "horizon", FORECAST_MAX_HORIZONS)
        var = np.zeros((K, self.L))
        _check(self._lib.moihgp_forecast_variances(self._h, hz, K, var.ctypes.data_as(c_double_p)), self._lib)
        return var

    def forecast_paths(self, x: Optional[torch.Tensor] = None, n: Optional[int] = None, nsamples: Optional[int] = None, seed: int = 0, sample0: int = 0,
                       latent0: int = 0, step0: int = 0, states: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       want_states: bool = True, stream=None):
        """Seeded joint draws of the n ticks beyond a stream for every latent (include/moihgp.h moihgp_forecast_paths): paths[s, l, j] is a draw of
        the OBSERVATION of latent l at tick T + step0 + j (noise included) given the ticks up to the end state and nothing else, with the GP
        predictive covariance across horizons (path_covariance()); the mean over draws is forecast_tail().  The draws are not jointly consistent with
        a sample() draw of the same stream.  Start: `x` [L, d], a stream's end state with the Kalman gains (forecast(), forecast_scores(), smooth()),
        shared by all samples -- or `states` [S, L, d] float64, the states an earlier call returned, with `step0` the number of steps already
        drawn: the calls then reproduce one long call bit for bit.  The noise is Philox4x32-10 keyed by `seed` and counted by
        (step0 + j, latent0 + l, sample0 + s), so ranges of samples or latents reproduce one large call too.

        Returns (paths [S, L, >=n], states [S, L, d] float64 or None, status [L] int32: 0 ok, 1 Kalman DARE not converged (rows and states NaN)).
        The dtype is x's, or `out`'s when `states` is given (float64 without `out`).  Asynchronous on the current torch stream.  `out` (optional)
        [S, L, >=n] as forecast()'s; it must not overlap x or the states."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= (1 << 20):
            raise ValueError(f"n {n!r} must be an integer in 0 .. 2^20")
        if isinstance(nsamples, bool) or not isinstance(nsamples, (int, np.integer)) or not 1 <= nsamples <= 65535:
            raise ValueError(f"nsamples {nsamples!r} must be an integer in 1 .. 65535")
        if isinstance(step0, bool) or not isinstance(step0, (int, np.integer)) or not 0 <= step0 <= (1 << 32) - n:
            raise ValueError(f"step0 {step0!r} must be an integer with 0 <= step0 and step0 + n <= 2^32")
        n, S, step0 = int(n), int(nsamples), int(step0)
        seed, sample0, latent0 = int(seed), int(sample0), int(latent0)
        if not (0 <= seed < 1 << 64 and 0 <= sample0 < 1 << 32 and 0 <= latent0 < 1 << 32):
            raise ValueError("seed must be in 0 .. 2^64 - 1, sample0 and latent0 in 0 .. 2^32 - 1")
        if (x is None) == (states is None):
            raise ValueError("exactly one of x and states must be given")
        if x is not None:
            if not x.is_cuda or x.dtype not in _DT or not x.is_contiguous() or tuple(x.shape) != (self.L, self.d):
                raise ValueError("x must be a contiguous CUDA tensor [L, d] (float32/float64)")
            dtype, device, start = x.dtype, x.device, x
        else:
            if not states.is_cuda or states.dtype != torch.float64 or not states.is_contiguous() or tuple(states.shape) != (S, self.L, self.d):
                raise ValueError("states must be a contiguous float64 CUDA tensor [S, L, d]")
            dtype, device, start = (torch.float64 if out is None else out.dtype), states.device, states
            if dtype not in _DT:
                raise ValueError("out must be float32 or float64")
        self._refuse_stacked("forecast_paths")
        if out is None:
            out = torch.empty((S, self.L, padded_len(max(n, 1), dtype)), dtype=dtype, device=device)[:, :, :n]
        ld_out, plane = _plane_strides(out, S, self.L, n, dtype, device)
        states_out = torch.empty((S, self.L, self.d), dtype=torch.float64, device=device) if want_states else None
        b0, b1 = out.data_ptr(), out.data_ptr() + ((S - 1) * plane + self.L * ld_out) * out.element_size()
        for t in (start, states_out):
            if t is not None and n > 0 and t.data_ptr() < b1 and b0 < t.data_ptr() + t.numel() * t.element_size():
                raise ValueError("out must not overlap x or the states")
        status = torch.empty((self.L,), dtype=torch.int32, device=device)
        rc = self._lib.moihgp_forecast_paths(self._h, _DT[dtype], C.c_void_p(x.data_ptr()) if x is not None else None,
                                             C.c_void_p(states.data_ptr()) if states is not None else None,
                                             C.c_void_p(states_out.data_ptr()) if want_states else None, n, step0, S, seed, sample0, latent0,
                                             C.c_void_p(out.data_ptr()), ld_out, plane, C.c_void_p(status.data_ptr()), _stream_ptr(stream))
        _check(rc, self._lib)
        return out, states_out, status

    def path_covariance(self, l: int, n: int):
        """(C [n, n], taps [n]) of latent l, fp64 numpy, on the host: the covariance across horizons of forecast_paths()' draws, C = Sv Lam Lam^T
        with Lam lower-triangular Toeplitz of the taps lam_0 = 1, lam_k = (A^k K)_0 and Sv = P_00 + R = P_00 / K_0 (latent(l)["A"] and
        smoother(l)).  Its diagonal is forecast_variances([j + 1]) + R; 1^T C 1 is the variance of the sum over the next n ticks.  NaN for a
        latent whose Kalman DARE did not converge."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= n <= (1 << 20):
            raise ValueError(f"n {n!r} must be an integer in 0 .. 2^20")
        n = int(n)
        self._refuse_stacked("path_covariance")
        A, sm = self.latent(int(l))["A"], self.smoother(int(l))
        if np.isnan(self.forecast_variances([1])[0, int(l)]):
            return np.full((n, n), np.nan), np.full(n, np.nan)
        K, Sv = sm["K"], sm["P"][0, 0] / sm["K"][0]
        taps, v = np.ones(n), K.copy()
        for k in range(1, n):
            v = A @ v
            taps[k] = v[0]
        Lam = np.zeros((n, n))
        for k in range(n):
            Lam[np.arange(k, n), np.arange(0, n - k)] = taps[k]
        return Sv * (Lam @ Lam.T), taps


def project_stream(gp, Y: torch.Tensor, stream=None) -> torch.Tensor:
    """OILMM projection of a tick-major observation stream Y [T, M] with the mixing of `gp`
    (a pywrapper.MOIHGP): returns the series-major projected stream [L, ld] (moihgp.h:181 per tick)."""
    lib = load_library()
    if not Y.is_cuda or Y.dtype not in _DT or Y.dim() != 2 or not Y.is_contiguous() or Y.shape[1] != gp.num_output:
        raise ValueError("Y must be a contiguous CUDA tensor [T, M]")
    T = Y.shape[0]
    Ty = alloc_stream(gp.num_latent, T, Y.dtype, Y.device)
    _check(lib.moihgp_project_stream(gp.handle, _DT[Y.dtype], C.c_void_p(Y.data_ptr()), T, C.c_void_p(Ty.data_ptr()),
                                     Ty.stride(0), _stream_ptr(stream)), lib)
    return Ty


def unproject_stream(gp, Tyhat: torch.Tensor, T: int, stream=None) -> torch.Tensor:
    """Yhat [T, M] = U S^1/2 Tyhat (moihgp.h:222-225 per tick) from a series-major stream [L, ld]."""
    lib = load_library()
    Yhat = torch.empty((T, gp.num_output), dtype=Tyhat.dtype, device=Tyhat.device)
    _check(lib.moihgp_unproject_stream(gp.handle, _DT[Tyhat.dtype], C.c_void_p(Tyhat.data_ptr()), T, Tyhat.stride(0),
                                       C.c_void_p(Yhat.data_ptr()), _stream_ptr(stream)), lib)
    return Yhat


def _check_observations(gp, Y: torch.Tensor):
    if not isinstance(Y, torch.Tensor) or not Y.is_cuda or Y.dtype not in _DT or Y.dim() != 2 or not Y.is_contiguous() or Y.shape[1] != gp.num_output:
        raise ValueError("Y must be a contiguous CUDA tensor [T, M] (float32/float64)")


def _check_tiled(name: str, Tt: torch.Tensor, L: int, T: int, dtype, device):
    """ValueError unless Tt is a contiguous, 16-byte aligned tensor [ceil(T / SEG), L, SEG] of `dtype` on `device`."""
    seg = seg_ticks(dtype)
    nseg = (T + seg - 1) // seg
    if (not isinstance(Tt, torch.Tensor) or Tt.device != device or Tt.dtype != dtype or not Tt.is_contiguous() or tuple(Tt.shape) != (nseg, L, seg)
            or Tt.data_ptr() % 16 != 0):
        raise ValueError(f"{name} must be a contiguous, 16-byte aligned {dtype} tensor [ceil(T / {seg}) = {nseg}, L = {L}, {seg}] on {device}")


def project_stream_tiled(gp, Y: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """`project_stream` with the result in the SEGMENT-MAJOR layout [ceil(T / SEG), L, SEG] that `LatentBank.filter_tiled` sweeps
    (moihgp_project_stream_tiled): the same arithmetic and the same values bit for bit, missing outputs included, without a `tile_stream` pass.
    `out` (optional) must be exactly that shape, contiguous, of Y's dtype and device.  Ticks past T in the last tile are not written: they keep
    whatever the buffer held (the sweep ignores them)."""
    lib = load_library()
    _check_observations(gp, Y)
    T, L = Y.shape[0], gp.num_latent
    if out is None:
        out = alloc_stream_tiled(L, T, Y.dtype, Y.device)
    _check_tiled("out", out, L, T, Y.dtype, Y.device)
    _check(lib.moihgp_project_stream_tiled(gp.handle, _DT[Y.dtype], C.c_void_p(Y.data_ptr()), T, C.c_void_p(out.data_ptr()), _stream_ptr(stream)), lib)
    return out


def unproject_stream_tiled(gp, Tt: torch.Tensor, T: int, stream=None) -> torch.Tensor:
    """`unproject_stream` from a SEGMENT-MAJOR stream [ceil(T / SEG), L, SEG], e.g. the yhat of `LatentBank.filter_tiled`
    (moihgp_unproject_stream_tiled): Yhat [T, M], the same values bit for bit, without an `untile_stream` pass.  Ticks past T in the last tile
    are never read (they may hold anything, NaN included)."""
    lib = load_library()
    if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 0:
        raise ValueError("T must be a non-negative integer")
    T = int(T)
    if not isinstance(Tt, torch.Tensor) or not Tt.is_cuda or Tt.dtype not in _DT:
        raise ValueError("Tt must be a CUDA tensor (float32/float64)")
    _check_tiled("Tt", Tt, gp.num_latent, T, Tt.dtype, Tt.device)
    Yhat = torch.empty((T, gp.num_output), dtype=Tt.dtype, device=Tt.device)
    _check(lib.moihgp_unproject_stream_tiled(gp.handle, _DT[Tt.dtype], C.c_void_p(Tt.data_ptr()), T, C.c_void_p(Yhat.data_ptr()), _stream_ptr(stream)), lib)
    return Yhat


AUTO_TILED_ABOVE = 1024     # filter_outputs(layout="auto"): above this many latents both layouts run the same one-wavefront-per-latent sweep kernel


def filter_outputs(gp, Y: torch.Tensor, layout: str = "auto", want_nll: bool = True, stream=None):
    """Filtered outputs of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a pywrapper.MOIHGP), from a
    zero state: project -> LatentBank.filter / filter_tiled -> un-project, asynchronous on the torch stream.

    Returns (Yhat [T, M] in Y's dtype, x [L, d] end state, nll [L] fp64 or None).  Yhat[t] is what `gp.step` returns at tick t of the loop
    `for y in Y: x, yhat = gp.step(x, y)`.  Ticks with missing outputs are projected as project_stream does it: a tick with more than 64 missing
    outputs or fewer than L observed ones is treated as missing as a whole.

    layout: "series" -- series-major streams throughout; "tiled" -- segment-major streams throughout (project_stream_tiled -> filter_tiled ->
    unproject_stream_tiled, no retile pass; stacked models raise MoihgpError with rc 3); "auto" -- tiled exactly when the model is not stacked
    and has more than 1024 latents, where both layouts run the same sweep kernel (bit-equal results) and the tiled one moves a cold stream
    faster; at fewer latents the series-major entry has time-split and team kernels the tiled one lacks, so "auto" stays series-major."""
    if layout not in ("auto", "series", "tiled"):
        raise ValueError('layout must be "auto", "series" or "tiled"')
    _check_observations(gp, Y)
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    if layout == "auto":
        layout = "tiled" if (not bank.stacked and bank.L > AUTO_TILED_ABOVE) else "series"
    # (the intermediate buffers and the zero start state belong to the stream the kernels run on)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        if layout == "tiled":
            Tt = project_stream_tiled(gp, Y, stream=stream)
            yhat, x, nll = bank.filter_tiled(Tt, T, want_nll=want_nll, stream=stream)
            return unproject_stream_tiled(gp, yhat, T, stream=stream), x, nll
        Ty = project_stream(gp, Y, stream=stream)
        yhat, x, nll = bank.filter(Ty, T=T, want_nll=want_nll, stream=stream)
        return unproject_stream(gp, yhat, T, stream=stream), x, nll


def _output_variances(gp, var: np.ndarray, bad, message: str) -> np.ndarray:
    """The tail of the *_outputs functions: MoihgpError(message) where `bad` says that a latent failed, else var_Y[..., m] = sum_l U[m, l]^2 S_l var[..., l]
    from the latents' variances var [L] or [K, L] and the mixing in gp.params."""
    if bad:
        raise MoihgpError(message, 1)
    M, L = gp.num_output, gp.num_latent
    prm = gp.params
    U, S = prm[:M * L].reshape(M, L), prm[M * L:M * L + L]
    w = S * var
    return (U ** 2) @ w if w.ndim == 1 else w @ (U ** 2).T      # (the two products as they have always been taken: no last-bit change)


def smooth_outputs(gp, Y: torch.Tensor, stream=None):
    """Smoothed outputs of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a pywrapper.MOIHGP):
    project_stream -> LatentBank.smooth -> unproject_stream, from a zero state.

    Returns (Ys [T, M] in Y's dtype, var_Y [M] fp64 numpy) with var_Y[m] = sum_l U[m, l]^2 S_l var_smoothed[l]: the steady-state posterior
    variance of the latent FUNCTION at output m (interior ticks), without the observation noise.  Raises MoihgpError if any latent's Kalman DARE
    did not converge (status 1).  Ticks with missing outputs are projected as project_stream does it: a tick with more than 64 missing outputs
    or fewer than L observed ones is treated as missing as a whole."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    ys, _, status = bank.smooth(Ty, T=T, stream=stream)
    Ys = unproject_stream(gp, ys, T, stream=stream)
    bad = int((status != 0).sum())      # (synchronises)
    return Ys, _output_variances(gp, bank.latent_variances()[1], bad, f"smooth_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows "
                                 "are NaN and so is every output that mixes them")


def smooth_outputs_exact(gp, Y: torch.Tensor, var_ticks=(0, -1), stream=None):
    """`smooth_outputs` with exact edges (LatentBank.smooth_exact): project_stream -> smooth_exact -> unproject_stream, from the prior.

    Returns (Ys [T, M] in Y's dtype, var_Y [len(var_ticks), M] fp64 numpy) with var_Y[k, m] = sum_l U[m, l]^2 S_l var[l, var_ticks[k]]: the
    posterior variance of the latent FUNCTION at output m and tick var_ticks[k] (negative ticks count from the end), without the observation
    noise.  For a gap-free series both are the GP posterior's at every tick.  Raises MoihgpError on any non-zero status (1 the Kalman DARE did
    not converge, 3 a latent's edges overlap in a series longer than 4096 ticks, 4 its edge tables failed).  Missing outputs are projected as
    in smooth_outputs."""
    T = Y.shape[0]
    ticks = [int(t) for t in var_ticks]
    if any(t < -T or t >= T for t in ticks):
        raise ValueError("var_ticks must lie in -T .. T - 1")
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    ys, var, _, status = bank.smooth_exact(Ty, T=T, stream=stream)
    Ys = unproject_stream(gp, ys, T, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        picked = var[:, ticks].to(torch.float64).T.contiguous().cpu().numpy() if ticks else np.zeros((0, bank.L))     # (synchronises)
        bad = int((status != 0).sum())
    return Ys, _output_variances(gp, picked, bad, f"smooth_outputs_exact: {bad} latent(s) have a non-zero status (1 Kalman DARE not converged, 3 edges "
                                 "overlap in a series longer than 4096 ticks, 4 edge tables failed)")


def posterior_outputs(gp, Y: torch.Tensor, var_ticks=(0, -1), stream=None):
    """The GP posterior of the outputs across missing ticks (LatentBank.posterior): project_stream -> posterior -> unproject_stream, from the prior.

    Returns (Ys [T, M] in Y's dtype, var_Y [len(var_ticks), M] fp64 numpy, nll [L] fp64 numpy) with var_Y[k, m] = sum_l U[m, l]^2 S_l
    var[l, var_ticks[k]]: the posterior variance of the latent FUNCTION at output m and tick var_ticks[k] (negative ticks count from the end),
    without the observation noise -- it widens inside a gap -- and nll the latents' exact -log marginal likelihoods of their projected
    streams.  Raises MoihgpError on any non-zero status (5: a latent's recursion broke down).  Missing outputs are projected as in
    smooth_outputs: a tick with more than 64 missing outputs or fewer than L observed ones is a missing tick of every latent."""
    T = Y.shape[0]
    ticks = [int(t) for t in var_ticks]
    if any(t < -T or t >= T for t in ticks):
        raise ValueError("var_ticks must lie in -T .. T - 1")
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    out = bank.posterior(Ty, T=T, stream=stream)
    Ys = unproject_stream(gp, out["mean"], T, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        picked = out["var"][:, ticks].to(torch.float64).T.contiguous().cpu().numpy() if ticks else np.zeros((0, bank.L))     # (synchronises)
        nll = out["nll"].cpu().numpy()
        bad = int((out["status"] != 0).sum())
    return Ys, _output_variances(gp, picked, bad, f"posterior_outputs: {bad} latent(s) have a non-zero status (5 the recursion broke down)"), nll


def sample_noise(seed: int, L: int, S: int, T: int, latent0: int = 0, sample0: int = 0, want_start: bool = True, device="cuda", stream=None):
    """The sampler's normals without a handle (moihgp_sample_noise): (noise [S, L, T] float32, start [S, L, 4] float32 or None) with noise[s, l, t]
    the normal of tick t, latent latent0 + l, sample sample0 + s, and start the four start normals.  The way to audit a draw."""
    lib = load_library()
    ld = padded_len(max(T, 1), torch.float32)
    noise = torch.empty((S, L, ld), dtype=torch.float32, device=device)      # (empty: nothing of torch's runs on a stream of its own here)
    start = torch.empty((S, L, 4), dtype=torch.float32, device=device) if want_start else None
    _check(lib.moihgp_sample_noise(int(seed), int(latent0), L, int(sample0), S, T, C.c_void_p(noise.data_ptr()), ld,
                                   C.c_void_p(start.data_ptr()) if want_start else None, _stream_ptr(stream)), lib)
    return noise[:, :, :T], start


def sample_outputs(gp, Y: torch.Tensor, nsamples: int, seed: int = 0, stream=None):
    """Joint posterior samples of the outputs for a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a
    pywrapper.MOIHGP), from a zero state: project_stream -> LatentBank.sample -> unproject_stream per plane (the latents are independent a
    posteriori, so un-projecting a plane of latent samples gives a joint sample of all outputs; of the function, without observation noise).

    Returns (Ys [S, T, M] in Y's dtype, Ymean [T, M] the smoothed outputs, var_Y [M] fp64 numpy as smooth_outputs).  Raises MoihgpError on any
    non-zero status (Kalman DARE not converged, or the sampler's realization not accepted).  Missing outputs as smooth_outputs."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    smp, ys, _, status = bank.sample(Ty, nsamples, seed=seed, T=T, stream=stream)
    Ys = torch.stack([unproject_stream(gp, smp[s], T, stream=stream) for s in range(smp.shape[0])])
    Ymean = unproject_stream(gp, ys, T, stream=stream)
    st = status.cpu().numpy()           # (synchronises)
    return Ys, Ymean, _output_variances(gp, bank.latent_variances()[1], st.any(), f"sample_outputs: {int((st == 1).sum())} latent(s) whose Kalman DARE "
                                        f"did not converge, {int((st == 2).sum())} whose sampling realization was not accepted; their rows are NaN and "
                                        "so is every output that mixes them")


def forecast_outputs(gp, Y: torch.Tensor, horizons, tail: int = 0, gains: str = "kalman", stream=None):
    """Forecasts of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a pywrapper.MOIHGP), from a zero
    state: project_stream -> LatentBank.forecast -> unproject_stream per horizon.

    Returns (Yf [K, T, M] in Y's dtype, var_Y [K, M] fp64 numpy, Ytail [tail, M] or None).  Yf[k, t] is the mean of the outputs at tick
    t + horizons[k] given the ticks <= t (stored at the tick the forecast is made at); Ytail[j] the mean at tick T + j given all T ticks.
    var_Y[k, m] = sum_l U[m, l]^2 S_l var[k, l]: the steady-state variance of the latent FUNCTION at output m, without the observation noise; it
    belongs to gains "kalman" and is returned unchanged with "handle", whose error it does not describe.  Raises MoihgpError if any latent's Kalman
    DARE did not converge.  Ticks with missing outputs are projected as project_stream does it: a tick with more than 64 missing outputs or fewer
    than L observed ones is treated as missing as a whole."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    _, K = _int_list(horizons, "horizon", FORECAST_MAX_HORIZONS)
    Ty = project_stream(gp, Y, stream=stream)
    fc, x, status = bank.forecast(Ty, horizons, T=T, gains=gains, stream=stream)
    Yf = torch.stack([unproject_stream(gp, fc[k], T, stream=stream) for k in range(K)])
    Ytail = None
    if tail:
        Ytail = unproject_stream(gp, bank.forecast_tail(x, tail, stream=stream), tail, stream=stream)
    var = bank.forecast_variances(horizons)      # (synchronises)
    bad = int(((status != 0).cpu().numpy() | np.isnan(var).any(axis=0)).sum())
    # (with gains "handle" the means exist, but var_Y does not)
    return Yf, _output_variances(gp, var, bad, f"forecast_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows and variances are NaN "
                                 "and so is every output that mixes them"), Ytail


def forecast_paths_noise(seed: int, L: int, S: int, n: int, step0: int = 0, latent0: int = 0, sample0: int = 0, device="cuda", stream=None) -> torch.Tensor:
    """The normals of LatentBank.forecast_paths without a handle (moihgp_forecast_paths_noise): noise [S, L, n] float32 with noise[s, l, j] the normal
    of step step0 + j, latent latent0 + l, sample sample0 + s.  The way to audit a path."""
    lib = load_library()
    ld = padded_len(max(n, 1), torch.float32)
    noise = torch.empty((S, L, ld), dtype=torch.float32, device=device)
    _check(lib.moihgp_forecast_paths_noise(int(seed), int(latent0), L, int(sample0), S, int(step0), int(n), C.c_void_p(noise.data_ptr()), ld,
                                           _stream_ptr(stream)), lib)
    return noise[:, :, :n]


def forecast_path_outputs(gp, Y: torch.Tensor, n: int, nsamples: int, seed: int = 0, stream=None):
    """Joint draws of the outputs at the n ticks beyond a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp`
    (a pywrapper.MOIHGP), from a zero state: project_stream -> the end state with the Kalman gains (forecast_scores, which writes no plane) ->
    LatentBank.forecast_paths -> unproject_stream per sample, and forecast_tail for the mean.

    Returns (Ypaths [S, n, M] in Y's dtype, Ymean [n, M]).  Ypaths[s, j] is a draw of the outputs' observation process at tick T + j inside the
    mixing's span, with the latents' noise (the sigma^2 component outside the span is not drawn); Ymean[j] the mean at tick T + j given all T
    ticks.  Raises MoihgpError if any latent's Kalman DARE did not converge.  Missing outputs as forecast_outputs."""
    _check_observations(gp, Y)
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    x = bank.forecast_scores(Ty, [1], T=Y.shape[0], stream=stream)["x"]
    paths, _, status = bank.forecast_paths(x, n, nsamples, seed=seed, want_states=False, stream=stream)
    Ypaths = torch.stack([unproject_stream(gp, paths[s], n, stream=stream) for s in range(paths.shape[0])])
    Ymean = unproject_stream(gp, bank.forecast_tail(x, n, stream=stream), n, stream=stream)
    bad = int((status != 0).sum())      # (synchronises)
    if bad:
        raise MoihgpError(f"forecast_path_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows are NaN and so is every output "
                          "that mixes them", 1)
    return Ypaths, Ymean


def score_summary(scores: dict) -> dict:
    """Per (horizon, latent) figures from the sums of LatentBank.forecast_scores / score_outputs: mse = sum_sq / n and bias = sum_err / n; where
    the dict holds pvar (gains "kalman") also smse = mse / pvar, which is ~ 1 for a calibrated model, and the mean log predictive density
    mlpd = -1/2 (log(2 pi pvar) + mse / pvar).  smse and mlpd are NaN for h = 0 (in-sample: pvar is not its variance) and wherever n = 0, as are
    mse and bias there.  At h = 1, -n mlpd is the steady-state Kalman negative log likelihood of the scored ticks.  Torch ops on the sums' own
    device, no synchronisation."""
    n = scores["n"].to(torch.float64)
    nan = torch.full_like(n, float("nan"))
    some = n > 0
    den = torch.where(some, n, torch.ones_like(n))
    out = dict(mse=torch.where(some, scores["sum_sq"] / den, nan), bias=torch.where(some, scores["sum_err"] / den, nan))
    pvar = scores.get("pvar")
    if pvar is not None:
        # (one fill per horizon: a host list copied to the device would wait for the stream)
        ahead = torch.cat([torch.full((1, 1), bool(h > 0), dtype=torch.bool, device=n.device) for h in scores["horizons"]]) & some
        out["smse"] = torch.where(ahead, out["mse"] / pvar, nan)
        out["mlpd"] = torch.where(ahead, -0.5 * (torch.log(2.0 * np.pi * pvar) + out["mse"] / pvar), nan)
    return out


def score_outputs(gp, Y: torch.Tensor, horizons, t_first: int = 0, gains: str = "kalman", stream=None) -> dict:
    """Forecast scores of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a pywrapper.MOIHGP), from
    a zero state: project_stream -> LatentBank.forecast_scores on the projected streams; returns that method's dict.  Ticks with missing outputs
    are projected as project_stream does it (forecast_outputs): a tick with more than 64 missing outputs or fewer than L observed ones is missing
    as a whole, and is then no target.

    The scores are those of the projected streams.  With orthonormal mixing columns and fully observed ticks, the squared forecast error of the
    outputs inside the mixing's span is sum_l S_l sum_sq[k, l]; that sum is stated here, not computed."""
    _check_observations(gp, Y)
    bank = LatentBank.from_handle(gp)
    Ty = project_stream(gp, Y, stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        return bank.forecast_scores(Ty, horizons, T=Y.shape[0], t_first=t_first, gains=gains, stream=stream)


def lagged_outputs(gp, Y: torch.Tensor, lags, stream=None):
    """Fixed-lag smoothed outputs of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a
    pywrapper.MOIHGP), from a zero state: project_stream -> LatentBank.lagged -> unproject_stream per lag.

    Returns (Yl [K, T, M] in Y's dtype, var_Y [K, M] fp64 numpy).  Yl[k, t] is the mean of the outputs at tick t given the ticks
    <= min(t + lags[k], T - 1).  var_Y[k, m] = sum_l U[m, l]^2 S_l var[k, l]: the steady-state variance of the latent FUNCTION at output m, without
    the observation noise.  Raises MoihgpError if any latent's Kalman DARE did not converge.  Ticks with missing outputs are projected as
    project_stream does it: a tick with more than 64 missing outputs or fewer than L observed ones is treated as missing as a whole."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    _, K = _int_list(lags, "lag", LAGGED_MAX_LAGS)
    Ty = project_stream(gp, Y, stream=stream)
    lg, _, _, status = bank.lagged(Ty, lags, T=T, stream=stream)
    Yl = torch.stack([unproject_stream(gp, lg[k], T, stream=stream) for k in range(K)])
    var = bank.lagged_variances(lags)      # (synchronises)
    bad = int(((status != 0).cpu().numpy() | np.isnan(var).any(axis=0)).sum())
    return Yl, _output_variances(gp, var, bad, f"lagged_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows and variances are NaN "
                                 "and so is every output that mixes them")


def interpolate_outputs(gp, Y: torch.Tensor, fracs, stream=None):
    """Smoothed outputs between the ticks of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a
    pywrapper.MOIHGP), from a zero state: project_stream -> LatentBank.interpolate -> unproject_stream per offset.

    Returns (Yfine [K, T, M] in Y's dtype, Ys [T, M] the smoothed outputs on the grid, var_fine [K, M], var_Y [M] fp64 numpy).  Yfine[k, t] is the
    mean of the outputs at time (t + fracs[k]) dt given all T ticks (its last row: the forecast fracs[k] dt past the end).  var_fine[k, m] =
    sum_l U[m, l]^2 S_l var[k, l] and var_Y as smooth_outputs': the steady-state variances of the latent FUNCTION at output m, without the observation
    noise.  Raises MoihgpError if any latent's Kalman DARE did not converge.  Ticks with missing outputs are projected as project_stream does it:
    a tick with more than 64 missing outputs or fewer than L observed ones is treated as missing as a whole."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    _, K = _frac_list(fracs)
    Ty = project_stream(gp, Y, stream=stream)
    fine, ys, _, status = bank.interpolate(Ty, fracs, T=T, stream=stream)
    Yfine = torch.stack([unproject_stream(gp, fine[k], T, stream=stream) for k in range(K)])
    Ys = unproject_stream(gp, ys, T, stream=stream)
    var = bank.interp_variances(fracs)      # (synchronises)
    bad = int(((status != 0).cpu().numpy() | np.isnan(var).any(axis=0)).sum())
    message = (f"interpolate_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows and variances are NaN and so is every output "
               "that mixes them")
    var_fine = _output_variances(gp, var, bad, message)
    return Yfine, Ys, var_fine, _output_variances(gp, bank.latent_variances()[1], bad, message)


def slope_outputs(gp, Y: torch.Tensor, fracs=(0.0,), given: str = "all", stream=None):
    """Rate of change of the outputs of a tick-major observation stream Y [T, M] (NaN = missing output) with the parameters of `gp` (a
    pywrapper.MOIHGP), from a zero state: project_stream -> LatentBank.slope -> unproject_stream per offset (the un-projection is linear, so the
    planes are the outputs' slopes).

    Returns (dY [K, T, M] in Y's dtype, var_dY [K, M] fp64 numpy).  dY[k, t] is the derivative with respect to time of the mean of the outputs at
    time (t + fracs[k]) dt given all T ticks (given = "all") or the ticks up to t ("past"); var_dY[k, m] = sum_l U[m, l]^2 S_l var[k, l] its
    steady-state variance.  Raises MoihgpError if any latent's Kalman DARE did not converge.  Ticks with missing outputs are projected as
    project_stream does it."""
    T = Y.shape[0]
    bank = LatentBank.from_handle(gp)
    _, K = _frac_list(fracs)
    Ty = project_stream(gp, Y, stream=stream)
    slope, _, _, status = bank.slope(Ty, fracs, given, T=T, stream=stream)
    dY = torch.stack([unproject_stream(gp, slope[k], T, stream=stream) for k in range(K)])
    var = bank.slope_variances(fracs, given)      # (synchronises)
    bad = int(((status != 0).cpu().numpy() | np.isnan(var).any(axis=0)).sum())
    return dY, _output_variances(gp, var, bad, f"slope_outputs: the Kalman DARE of {bad} latent(s) did not converge; their rows and variances are NaN "
                                 "and so is every output that mixes them")


def upsample_outputs(gp, Y: torch.Tensor, factor: int, stream=None):
    """The smoothed outputs of Y [T, M] on a grid `factor` times as fine (2 .. 9): interpolate_outputs at the offsets j / factor, interleaved with
    the smoothed outputs on the grid by torch ops.

    Returns (Yup [(T - 1) factor + 1, M] with Yup[t factor + j] the mean at time (t + j / factor) dt -- the points past the last tick are dropped --
    and var_up [factor, M] fp64 numpy, the steady-state variance of the latent function at offset j / factor: var_up[0] is smooth_outputs' var_Y)."""
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= factor <= INTERP_MAX_POINTS + 1:
        raise ValueError(f"factor {factor!r} must be an integer in 2 .. {INTERP_MAX_POINTS + 1}")
    factor = int(factor)
    T, M = Y.shape[0], Y.shape[1]
    Yfine, Ys, var_fine, var_Y = interpolate_outputs(gp, Y, [j / factor for j in range(1, factor)], stream=stream)
    with torch.cuda.stream(torch.cuda.current_stream() if stream is None else stream):
        Yup = torch.cat([Ys[None], Yfine]).permute(1, 0, 2).reshape(T * factor, M)[:max((T - 1) * factor + 1, 0)]
    return Yup, np.concatenate([var_Y[None], var_fine])
