"""Plumbing of the whole-stream sweep tests (smoother, forecasts, forecast scores, sampler, fixed-lag, off-grid, slopes, slow latents): the
parameter pool and shapes, the one `env` fixture, bank builders, device buffers with guarded padding, the three gap patterns, the end-to-end
draw, the g++ build of a tests/cxx binary and the header / loader / export checks.  Test modules import from here (and the numpy definitions
from stream_reference), never from each other.  pytest does not rewrite the asserts of this module, so each carries its own message."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from parity_support import FP32_TOL, FP64_TIGHT, KMAP  # noqa: F401  (the project's tolerances and kernel names, re-exported)
from stream_reference import F_of, gain_tables, tables

POOL = [(1.0, 1.0, 0.1), (0.5, 0.6, 0.02), (2.0, 1.7, 0.3), (1.3, 0.8, 1e-6), (0.8, 2.0, 0.05), (1.6, 0.5, 0.2), (0.7, 1.2, 0.01), (1.1, 0.9, 1e-3)]
CASES = [(L, T) for L in (1, 7, 256) for T in (1, 2, 63, 1000, 10037)] + [(4096, 63), (4096, 1000)]
HMAX = 1 << 20        # the largest horizon a forecast call takes
LMAX = 1 << 20        # the largest lag
LAGS8 = [0, 1, 15, 16, 17, 1023, 1024, LMAX]      # the chunk and segment edges of the shifted read, and a lag past the end
POISON = 1e30
DT = 0.1
FRACS1 = [0.5]                                              # one plane per replay
FRACS3 = [0.25, 0.5, 0.75]                                  # two per replay, and a repeated replay whose second plane is idle
FRACS8 = [0.0, 0.125, 0.9, 0.5, 0.25, 0.999, 0.75, 1e-3]    # four full replays, offset 0 among them
# The off-grid variance (P_phi + G_phi (Ps - P) G_phi^T)_00 is a difference of terms of the size of P_00 and goes through P^-1, so an fp64 evaluation carries
# a relative rounding error of the order of eps cond(P) P_00 / var.  On POOL's draw (1.3, 0.8, 1e-6) that is 3e-8 (eps = 2.2e-16, cond(P) = 1.5e4, P_00 = 9e-3,
# var = 1e-6 near a tick), 1e-11 and less on the others.  Held against an 80-bit evaluation of the same formula, the numpy reference is good to 3e-12
# over the whole POOL at the offsets VAR_INNER, but only to 5e-10 at VAR_EDGE (beside a tick, where var falls to var_smoothed): the library's
# variances are compared at 1e-10 where the reference supports that, and at the rounding bound of the formula elsewhere.
VAR_INNER = [0.125, 0.25, 0.5, 0.75]
VAR_EDGE = [0.0, 1e-3, 0.9, 0.999]


@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import streams
    return dict(torch=torch, streams=streams)


def tol_of(dtype):
    return FP64_TIGHT if dtype == "f64" else FP32_TOL


def tdt_of(torch, dtype):
    return torch.float64 if dtype == "f64" else torch.float32


def round32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ banks and their numpy tables
def bank_of(streams, kern, L, builder, dt=0.1, pool=POOL):
    """A bank of L latents that cycle through `pool`, one numpy table dict per latent from builder(kern, dt, prm), and the parameters [L][3]."""
    prm = np.array([pool[l % len(pool)] for l in range(L)], dtype=np.float64)
    tbs = {p: builder(kern, dt, p) for p in pool}
    return streams.LatentBank(dt, prm, kernel=KMAP[kern]), [tbs[pool[l % len(pool)]] for l in range(L)], prm


def bank_and_tables(streams, kern, L, dt=0.1, pool=POOL):
    return bank_of(streams, kern, L, tables, dt, pool)


def make_bank(streams, kern, L, gains, dt=0.1, pool=POOL):
    return bank_of(streams, kern, L, lambda k, d, p: gain_tables(k, d, p, gains), dt, pool)


_MODEL = {}


def model_of(kern, prm, dt=DT):
    """(tables, F) of one parameter draw, computed once."""
    key = (kern, tuple(prm), dt)
    if key not in _MODEL:
        _MODEL[key] = (tables(kern, dt, prm), F_of(kern, dt, prm))
    return _MODEL[key]


def pool_models(kern, L):
    ms = [model_of(kern, POOL[l % len(POOL)]) for l in range(L)]
    return [m[0] for m in ms], [m[1] for m in ms]


# ------------------------------------------------------------------------------------------------ device buffers
def to_dev(torch, a, dtype, T):
    """[L, T] view of a buffer whose row padding holds NaN."""
    buf = torch.full((a.shape[0], (T + 3) // 4 * 4 + 4), float("nan"), dtype=dtype, device="cuda")
    buf[:, :T] = torch.from_numpy(a).to(dtype)
    return buf[:, :T]


def to_dev_poison(torch, a, dtype, T):
    """[L, T] view of a slab filled with a finite poison: the row padding and a whole row past the last latent hold 1e30."""
    L = a.shape[0]
    buf = torch.full((L + 1, (T + 3) // 4 * 4 + 4), POISON, dtype=dtype, device="cuda")
    buf[:L, :T] = torch.from_numpy(a).to(dtype)
    return buf[:L, :T]


def sentinel_out(torch, K, L, T, tdt, pad_row=8, pad_plane=12):
    """[K, L, T] view with ld_out = T rounded up + pad_row and plane_stride = L * ld_out + pad_plane inside a slab filled with a sentinel."""
    ldo = (T + 3) // 4 * 4 + pad_row
    plane = L * ldo + pad_plane
    slab = torch.full((K * plane + 16,), 12345.0, dtype=tdt, device="cuda")
    return slab, torch.as_strided(slab, (K, L, T), (plane, ldo, 1), 0)


def padding_untouched(torch, slab, view):
    mask = torch.ones_like(slab, dtype=torch.bool)
    torch.as_strided(mask, view.shape, view.stride(), 0).fill_(False)
    return bool((slab[mask] == 12345.0).all())


def plane_err(got, ref, scale, floor=1e-6):
    """Worst row of max|got - ref| over the latent's h = 0 scale: forecasts decay with h, so a row is not normalised by its own size."""
    den = np.maximum(scale, floor * max(float(np.max(scale)), 1e-300))
    with np.errstate(invalid="ignore"):
        return float(np.max(np.max(np.abs(got - ref), axis=-1) / den))


# ------------------------------------------------------------------------------------------------ missing ticks: three patterns, three draws
def gaps_ends_run_copy(Ty, rng):
    """Returns a copy of Ty (the argument is left as it was) with NaNs at tick 0, at T-1, in a run of 20 (where the stream holds one) and at
    1 % scattered."""
    L, T = Ty.shape
    Ty = Ty.copy()
    Ty[:, 0] = np.nan; Ty[:, T - 1] = np.nan
    if T >= 63:
        Ty[::2, T // 3:T // 3 + 20] = np.nan
    Ty[rng.random((L, T)) < 0.01] = np.nan
    return Ty


def gaps_edges_blocks_inplace(Ty, rng):
    """Writes into Ty itself and returns it: missing ticks at the two ends, on both sides of a chunk edge and of a segment edge, one whole chunk,
    one whole segment, and 1 % scattered (whatever of these the stream is long enough for)."""
    L, T = Ty.shape
    Ty[:, 0] = np.nan; Ty[:, T - 1] = np.nan
    for t in (15, 16, 1023, 1024):
        if t < T:
            Ty[:, t] = np.nan
    if T >= 63:
        Ty[::2, 32:48] = np.nan
        Ty[rng.random((L, T)) < 0.01] = np.nan
    if T >= 2048:
        Ty[1::2, 1024:2048] = np.nan
    return Ty


def gaps_edges_inplace(Ty, rng):
    """Writes into Ty itself and returns it: missing ticks at the two ends, on both sides of a chunk edge and of a segment edge (where the stream
    has them), and 1 % scattered."""
    L, T = Ty.shape
    for t in (0, T - 1, 15, 16, 1023, 1024):
        if t < T:
            Ty[:, t] = np.nan
    Ty[rng.random((L, T)) < 0.01] = np.nan
    return Ty


# ------------------------------------------------------------------------------------------------ end to end: a full model and its observations
def end_to_end_inputs(rng, M, L, T, missing):
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05],
                             np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)]).ravel()])
    Y = np.sin(0.02 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :] % 5)) + 0.1 * rng.standard_normal((T, M))
    if missing:
        Y[rng.random((T, M)) < 0.02] = np.nan
    return params, Y


# ------------------------------------------------------------------------------------------------ C++ surface
def cxx_test_binary(hip_built, name):
    """Builds tests/cxx/<name>.cpp against the library into build/cxx_tests and returns the program's path."""
    build = os.path.join(ROOT, "build", "cxx_tests")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, name)
    libdir = os.path.dirname(hip_built)
    subprocess.run(["g++", "-std=c++14", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cxx", name + ".cpp"),
                    "-o", exe, "-L", libdir, "-lmoihgp", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def cxx_fmt(a):
    return " ".join("nan" if np.isnan(v) else repr(float(v)) for v in np.ravel(a))


def cxx_run(exe, inp):
    """The lines a test program prints for the input `inp`."""
    return subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.strip().split("\n")


def cxx_rows(lines):
    return np.array([[float(v) for v in line.split()] for line in lines])


# ------------------------------------------------------------------------------------------------ the C ABI's additive symbols
def assert_declared(symbols):
    """include/moihgp.h declares every symbol and the loader lists it; returns the header's text without its comments."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "moihgp.h")).read(), flags=re.S)
    from multioutputihgp_amd import _lib
    for n in symbols:
        assert re.search(r"\b%s\s*\(" % n, src), "%s is not declared in include/moihgp.h" % n
        assert n in _lib.ADDITIVE_SYMBOLS, "%s is not in _lib.ADDITIVE_SYMBOLS" % n
    return src


def assert_exported(hip_built, symbols):
    lib = C.CDLL(hip_built)
    for n in symbols:
        assert hasattr(lib, n), "%s is not exported by %s" % (n, hip_built)
