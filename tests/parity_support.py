"""Shared by the filter / gradient family of tests (test_gpu_parity and the modules that draw their cases the way it does) and by the tools
that replay its cases: the suite's stream and parameter draws, the padded device stream, the tolerances and the `env` fixture of that family
(another dict than the whole-stream sweeps' one in stream_support).  pytest does not rewrite the asserts of this module, so each carries its
own message."""
import numpy as np
import pytest

FP64_TOL = 1e-6      # the bar
FP64_TIGHT = 1e-9    # what we actually expect from fp64 (rounding-order differences only)
FP32_TOL = 1e-3
KMAP = {"Matern32": "Matern32", "Matern52": "Matern52ss"}   # oracle kernel -> product kernel name
STACKED = ["Matern32x2", "Matern52x2", "Matern52x3", "Matern52x4", "Matern32x4", "Matern32x3"]


@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import MOIHGP, load_library
    from multioutputihgp_amd import streams
    from oracle import cref
    lib = load_library()
    assert lib.moihgp_device_count() >= 1, "the library sees no device"
    return dict(MOIHGP=MOIHGP, streams=streams, cref=cref, lib=lib)


def synth(L, T, rng, nan_frac=0.0):
    """The suite's stream: one sinusoid per latent plus noise, with a share nan_frac of the ticks missing."""
    t = np.arange(T)[None, :]; l = np.arange(L)[:, None]
    Ty = np.sin(0.05 * t * (1 + l % 7)) + 0.1 * rng.standard_normal((L, T))
    if nan_frac:
        Ty[rng.random((L, T)) < nan_frac] = np.nan
    return Ty


def synth_params(L, rng):
    return np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])


def synth_params_stacked(L, J, rng):
    cols = []
    for _ in range(J):
        cols += [rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L)]
    return np.column_stack(cols + [rng.uniform(0.05, 0.2, L)])


def to_dev(a, dtype):
    """numpy [L, T] -> cuda [L, ld] padded per the alignment contract."""
    import torch
    from multioutputihgp_amd.streams import alloc_stream
    L, T = a.shape
    t = alloc_stream(L, T, dtype)
    t.zero_()
    t[:, :T] = torch.from_numpy(a).to(dtype)
    return t
