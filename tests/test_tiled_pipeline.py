"""Segment-major streams straight out of the projection and into the un-projection: moihgp_project_stream_tiled,
moihgp_unproject_stream_tiled, streams.filter_outputs and MOIHGPRegression::predictStream.

The tiled entries run the kernels of the series-major ones with another base pointer and leading dimension per tile -- the same operations
in the same order -- so wherever both layouts exist the comparison is np.array_equal, not a tolerance.  The tolerances that do appear are
those of the existing tests of the same quantities (test_project_unproject_stream, test_segment_major_streams_equal_series_major,
test_cxx_predict_smoothed_matches_python)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, rel_err
from stream_support import KMAP, cxx_test_binary

NEW_SYMBOLS = ("moihgp_project_stream_tiled", "moihgp_unproject_stream_tiled")
SHAPES = [(3, 1), (101, 70), (96, 64), (260, 130)]      # (M, L): one latent; odd ldb, scalar loads; vector loads; a partial second row tile
SENTINEL = 12345.0


# ------------------------------------------------------------------------------------------------ CPU: the ABI
def test_header_declares_the_tiled_products():
    src = open(os.path.join(ROOT, "include", "moihgp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name


def test_loader_lists_the_tiled_products():
    from multioutputihgp_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.ADDITIVE_SYMBOLS


def test_library_exports_the_tiled_products(hip_built):
    import ctypes as C
    lib = C.CDLL(hip_built)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    from multioutputihgp_amd import load_library
    loaded = load_library()
    for name in NEW_SYMBOLS:
        assert getattr(loaded, name).argtypes is not None and len(getattr(loaded, name).argtypes) == 6


def test_cxx_predict_stream_compiles_and_links(hip_built):
    assert os.path.exists(cxx_test_binary(hip_built, "predict_stream_test"))


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def env(hip_built):
    import torch
    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    torch.cuda.set_device(0)
    from multioutputihgp_amd import MOIHGP, MoihgpError
    from multioutputihgp_amd import streams
    return dict(torch=torch, MOIHGP=MOIHGP, MoihgpError=MoihgpError, streams=streams)


def _dtypes(env):
    return {"fp64": env["torch"].float64, "fp32": env["torch"].float32}


def _igp_params(L, rng):
    return np.column_stack([rng.uniform(0.5, 2, L), rng.uniform(0.5, 2, L), rng.uniform(0.05, 0.2, L)])


def _model(env, M, L, kern, rng):
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    gp.update(np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.03], _igp_params(L, rng).ravel()]))
    p = gp.params
    return gp, p[:M * L].reshape(M, L), p[M * L:M * L + L]


_MODELS = {}


def _shared_model(env, M, L):
    """One model per shape for the projection tests (built once, never modified)."""
    if (M, L) not in _MODELS:
        _MODELS[(M, L)] = _model(env, M, L, "Matern32", np.random.default_rng(100 * M + L))
    return _MODELS[(M, L)]


def _lengths(seg):
    return [1, seg - 1, seg, seg + 1, 2 * seg + 77]


def _payload(Tt, T):
    """[L, T] numpy view of the ticks < T of a segment-major tensor [nseg, L, seg]."""
    nseg, L, seg = Tt.shape
    return Tt.permute(1, 0, 2).reshape(L, nseg * seg)[:, :T].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_tiled_projection_is_the_series_major_one_bit_for_bit(env, dt, M, L):
    """project_stream_tiled == tile_stream(project_stream) on every tick < T (the same kernel arithmetic in the same order, other store addresses),
    and == numpy (Y U S^-1/2)^T at test_project_unproject_stream's tolerances; the buffer behind the stream (a spare tile) and the ticks >= T of
    the last tile are never stored to."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    seg = S.seg_ticks(dtype)
    gp, U, Sv = _shared_model(env, M, L)
    rng = np.random.default_rng(M + L)
    for T in _lengths(seg):
        nseg = (T + seg - 1) // seg
        Y = rng.standard_normal((T, M))
        Yd = torch.from_numpy(Y).to(dtype).cuda()
        buf = torch.full((nseg + 1, L, seg), SENTINEL, dtype=dtype, device="cuda")
        got = S.project_stream_tiled(gp, Yd, out=buf[:nseg])
        assert got.data_ptr() == buf.data_ptr() and tuple(got.shape) == (nseg, L, seg)
        want = S.tile_stream(S.project_stream(gp, Yd), T)
        fresh = S.project_stream_tiled(gp, Yd)
        torch.cuda.synchronize()
        a, b, c = _payload(got, T), _payload(want, T), _payload(fresh, T)
        assert a.shape == (L, T)
        assert np.array_equal(a, b), (T, float(np.abs(a - b).max()))
        assert np.array_equal(c, b), T
        ref = (Y @ U / np.sqrt(Sv)).T
        assert rel_err(a, ref) < (1e-12 if dtype == torch.float64 else 1e-5), T
        assert bool((buf[nseg] == SENTINEL).all()), ("stored behind the stream", T)
        tail = buf[:nseg].permute(1, 0, 2).reshape(L, nseg * seg)[:, T:]
        assert bool((tail == SENTINEL).all()), ("stored past T in the last tile", T)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_tiled_projection_with_missing_outputs(env, dt):
    """The recipe of test_project_stream_with_missing_outputs on a stream that crosses a segment boundary: a quarter of the ticks hold 1 .. 40
    NaNs, among them the last tick of tile 0, the first of tile 1 and the last of the stream; one tick has more than 64 missing outputs (its
    NaN column stands).  The least-squares kernel stores through the tiled address function: equal to the series-major projection bit for bit."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    seg = S.seg_ticks(dtype)
    M, L, T = 200, 100, seg + 40
    rng = np.random.default_rng(M + L + T)
    gp, _, _ = _model(env, M, L, "Matern52", rng)
    Y = rng.standard_normal((T, M))
    hit = set(int(t) for t in rng.choice(T, size=T // 4, replace=False)) | {seg - 1, seg, T - 1}
    big = 7
    hit.discard(big)
    for t in sorted(hit):
        k = int(rng.integers(1, 41))
        Y[t, rng.choice(M, size=k, replace=False)] = np.nan
    Y[big, rng.choice(M, size=70, replace=False)] = np.nan          # > 64 missing: beyond the least-squares path
    Yd = torch.from_numpy(Y).to(dtype).cuda()
    series = S.project_stream(gp, Yd)
    tiled = S.project_stream_tiled(gp, Yd)
    torch.cuda.synchronize()
    a, b = _payload(tiled, T), series[:, :T].cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True)
    assert np.isfinite(a[np.isfinite(b)]).all() and np.array_equal(np.isfinite(a), np.isfinite(b))
    cols = np.isnan(b).all(axis=0)
    assert list(np.nonzero(cols)[0]) == [big] and np.isfinite(b[:, sorted(hit)]).all()      # (the series-major side is what the recipe expects)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("M,L", SHAPES)
def test_tiled_unprojection_is_the_series_major_one_bit_for_bit(env, dt, M, L):
    """unproject_stream_tiled == unproject_stream(untile_stream) with NaN in the ticks >= T of the last tile: they never reach a stored row."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    seg = S.seg_ticks(dtype)
    gp, U, Sv = _shared_model(env, M, L)
    gen = torch.Generator("cuda").manual_seed(M * L)
    for T in _lengths(seg):
        nseg = (T + seg - 1) // seg
        flat = torch.randn((L, nseg * seg), dtype=dtype, device="cuda", generator=gen)      # [L, ticks] with NaN from tick T on
        flat[:, T:] = float("nan")
        Tt = flat.reshape(L, nseg, seg).permute(1, 0, 2).contiguous()
        assert T == nseg * seg or bool(torch.isnan(Tt[-1, :, T - (nseg - 1) * seg:]).all())
        got = S.unproject_stream_tiled(gp, Tt, T)
        want = S.unproject_stream(gp, S.untile_stream(Tt, T), T)
        torch.cuda.synchronize()
        a, b = got.cpu().numpy(), want.cpu().numpy()
        assert a.shape == (T, M) and np.isfinite(a).all(), T
        assert np.array_equal(a, b), (T, float(np.abs(a - b).max()))
        ref = (flat[:, :T].double().cpu().numpy().T * np.sqrt(Sv)) @ U.T
        assert rel_err(a, ref) < (1e-11 if dtype == torch.float64 else 1e-4), T      # (test_project_unproject_stream: ten times the projection's bar)


def _count_calls(monkeypatch, cls, name):
    calls = []
    orig = getattr(cls, name)

    def wrapper(self, *a, **kw):
        calls.append(1)
        return orig(self, *a, **kw)
    monkeypatch.setattr(cls, name, wrapper)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_filter_outputs_many_latents(env, monkeypatch, dt, kern):
    """Above 1024 latents both layouts run the same one-wavefront-per-latent sweep: "tiled" and "series" are bit-equal end to end, and "auto" is
    the tiled route."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    M, L, T = 1040, 1030, S.seg_ticks(dtype) + 300
    rng = np.random.default_rng(T)
    gp, _, _ = _model(env, M, L, kern, rng)
    Y = torch.from_numpy(np.sin(0.02 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :] % 5)) + 0.1 * rng.standard_normal((T, M))).to(dtype).cuda()
    ya, xa, na = S.filter_outputs(gp, Y, layout="series")
    calls = _count_calls(monkeypatch, S.LatentBank, "filter_tiled")
    yb, xb, nb = S.filter_outputs(gp, Y, layout="tiled")
    assert len(calls) == 1
    yc, xc, nc = S.filter_outputs(gp, Y)                       # "auto"
    assert len(calls) == 2
    yd, xd, nd = S.filter_outputs(gp, Y, want_nll=False)
    torch.cuda.synchronize()
    assert tuple(ya.shape) == (T, M) and tuple(xa.shape) == (L, gp.igp_dim) and tuple(na.shape) == (L,) and nd is None
    assert bool(torch.isfinite(ya).all())
    for y, x, n in ((yb, xb, nb), (yc, xc, nc)):
        assert np.array_equal(y.cpu().numpy(), ya.cpu().numpy())
        assert np.array_equal(x.cpu().numpy(), xa.cpu().numpy()) and np.array_equal(n.cpu().numpy(), na.cpu().numpy())
    assert np.array_equal(yd.cpu().numpy(), ya.cpu().numpy())


@pytest.mark.gpu
def test_filter_outputs_auto_is_series_major_at_few_latents(env, monkeypatch):
    torch, S = env["torch"], env["streams"]
    gp, _, _ = _model(env, 8, 4, "Matern52", np.random.default_rng(1))
    Y = torch.from_numpy(np.random.default_rng(2).standard_normal((50, 8))).cuda()
    tiled_calls = _count_calls(monkeypatch, S.LatentBank, "filter_tiled")
    series_calls = _count_calls(monkeypatch, S.LatentBank, "filter")
    S.filter_outputs(gp, Y)
    torch.cuda.synchronize()
    assert len(tiled_calls) == 0 and len(series_calls) == 1
    with pytest.raises(ValueError):
        S.filter_outputs(gp, Y, layout="segments")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
def test_filter_outputs_few_latents(env, dt, kern):
    """Few latents: the series-major sweep may split a stream over wavefronts (another summation order), so the layouts agree to the few-latent
    tolerances of test_segment_major_streams_equal_series_major; the first ticks equal the per-tick ABI as in test_project_unproject_stream."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    M, L, T = 12, 4, 300
    rng = np.random.default_rng(T)
    gp, _, _ = _model(env, M, L, kern, rng)
    Y = np.sin(0.02 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :] % 5)) + 0.1 * rng.standard_normal((T, M))
    Yd = torch.from_numpy(Y).to(dtype).cuda()
    ya, xa, na = S.filter_outputs(gp, Yd, layout="series")
    yb, xb, nb = S.filter_outputs(gp, Yd, layout="tiled")
    torch.cuda.synchronize()
    tol = 1e-11 if dtype == torch.float64 else 2e-4
    assert rel_err(yb.cpu().numpy(), ya.cpu().numpy()) < tol
    assert rel_err(xb.cpu().numpy(), xa.cpu().numpy()) < tol and rel_err(nb.cpu().numpy(), na.cpu().numpy()) < tol
    x = np.zeros((L, gp.igp_dim))
    for t in range(20):
        x, yh = gp.step(x, Y[t])
        for got in (ya, yb):
            assert rel_err(got[t].cpu().numpy(), yh) < (1e-10 if dtype == torch.float64 else 1e-4), t


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_filter_outputs_stacked_model(env, dt):
    """Stacked models have no segment-major sweep: "tiled" raises the library's rc 3, "auto" takes the series-major route."""
    torch, S = env["torch"], env["streams"]
    dtype = _dtypes(env)[dt]
    M, L, T = 12, 4, 300
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern52x2")
    Y = torch.from_numpy(np.random.default_rng(5).standard_normal((T, M))).to(dtype).cuda()
    with pytest.raises(env["MoihgpError"]) as ei:
        S.filter_outputs(gp, Y, layout="tiled")
    assert ei.value.rc == 3
    ya, xa, na = S.filter_outputs(gp, Y)
    yb, xb, nb = S.filter_outputs(gp, Y, layout="series")
    torch.cuda.synchronize()
    assert tuple(ya.shape) == (T, M) and bool(torch.isfinite(ya).all())
    assert np.array_equal(ya.cpu().numpy(), yb.cpu().numpy()) and np.array_equal(na.cpu().numpy(), nb.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["series", "tiled"])
def test_filter_outputs_on_a_side_stream(env, layout):
    """The whole pipeline on a non-default torch stream, synchronised only at its end."""
    torch, S = env["torch"], env["streams"]
    M, L, T = 96, 64, S.seg_ticks(torch.float32) + 100
    rng = np.random.default_rng(9)
    gp, _, _ = _model(env, M, L, "Matern52", rng)
    Y = torch.from_numpy(rng.standard_normal((T, M))).float().cuda()
    y0, x0, n0 = S.filter_outputs(gp, Y, layout=layout)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    y1, x1, n1 = S.filter_outputs(gp, Y, layout=layout, stream=side)
    side.synchronize()
    assert np.array_equal(y1.cpu().numpy(), y0.cpu().numpy())
    assert np.array_equal(x1.cpu().numpy(), x0.cpu().numpy()) and np.array_equal(n1.cpu().numpy(), n0.cpu().numpy())


@pytest.mark.gpu
def test_tiled_entries_validate_their_tensors(env):
    """Wrong dtype, shape, contiguity or segment count: ValueError before the library is called, and nothing is written."""
    torch, S = env["torch"], env["streams"]
    M, L = 8, 4
    gp, _, _ = _model(env, M, L, "Matern32", np.random.default_rng(3))
    seg = S.seg_ticks(torch.float32)
    T = seg + 5
    Y = torch.randn((T, M), dtype=torch.float32, device="cuda")
    good = lambda: torch.full((2, L, seg), SENTINEL, dtype=torch.float32, device="cuda")
    wide = torch.full((2, L, 2 * seg), SENTINEL, dtype=torch.float32, device="cuda")
    bad_outs = {
        "dtype": torch.full((2, L, seg), SENTINEL, dtype=torch.float64, device="cuda"),
        "nseg short": torch.full((1, L, seg), SENTINEL, dtype=torch.float32, device="cuda"),
        "nseg long": torch.full((3, L, seg), SENTINEL, dtype=torch.float32, device="cuda"),
        "L": torch.full((2, L + 1, seg), SENTINEL, dtype=torch.float32, device="cuda"),
        "seg": torch.full((2, L, seg // 2), SENTINEL, dtype=torch.float32, device="cuda"),
        "non-contiguous": wide[:, :, ::2],
        "2-d": torch.full((2 * L, seg), SENTINEL, dtype=torch.float32, device="cuda"),
        "host": torch.full((2, L, seg), SENTINEL, dtype=torch.float32),
    }
    for why, out in bad_outs.items():
        with pytest.raises(ValueError):
            S.project_stream_tiled(gp, Y, out=out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), why
    assert bool((wide == SENTINEL).all())
    for why, Yb in {"dtype": Y.half(), "M": Y[:, :M - 1].contiguous(), "non-contiguous": torch.randn((M, T), dtype=torch.float32, device="cuda").T,
                    "1-d": Y[0], "host": Y.cpu()}.items():
        out = good()
        with pytest.raises(ValueError):
            S.project_stream_tiled(gp, Yb, out=out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), why
    Tt = S.project_stream_tiled(gp, Y)
    torch.cuda.synchronize()
    keep = Tt.clone()
    for why, (bad, Tb) in {"T in another segment count": (Tt, seg), "T too long": (Tt, 2 * seg + 1), "negative T": (Tt, -1), "T not an integer": (Tt, 1.5),
                           "dtype": (Tt.half(), T), "L": (Tt[:, :L - 1].contiguous(), T), "non-contiguous": (Tt[:, :, ::2], T),
                           "seg": (Tt[:, :, :seg // 2].contiguous(), T), "host": (Tt.cpu(), T), "2-d": (Tt.reshape(2 * L, seg), T)}.items():
        with pytest.raises(ValueError):
            S.unproject_stream_tiled(gp, bad, Tb)
    torch.cuda.synchronize()
    assert np.array_equal(Tt.cpu().numpy(), keep.cpu().numpy(), equal_nan=True)
    # the C entries themselves: dtype, null pointers and the base's alignment are refused with rc 1; T == 0 is a no-op
    import ctypes as C
    from multioutputihgp_amd import load_library
    lib = load_library()
    out = good()
    yp, op, st = C.c_void_p(Y.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Yh = torch.full((T, M), SENTINEL, dtype=torch.float32, device="cuda")
    assert lib.moihgp_project_stream_tiled(gp.handle, 7, yp, T, op, st) == 1
    assert lib.moihgp_project_stream_tiled(gp.handle, 1, None, T, op, st) == 1
    assert lib.moihgp_project_stream_tiled(gp.handle, 1, yp, T, None, st) == 1
    assert lib.moihgp_project_stream_tiled(gp.handle, 1, yp, T, C.c_void_p(out.data_ptr() + 4), st) == 1
    assert lib.moihgp_project_stream_tiled(None, 1, yp, T, op, st) == 1
    assert lib.moihgp_project_stream_tiled(gp.handle, 1, yp, 0, op, st) == 0
    assert lib.moihgp_unproject_stream_tiled(gp.handle, 7, op, T, C.c_void_p(Yh.data_ptr()), st) == 1
    assert lib.moihgp_unproject_stream_tiled(gp.handle, 1, None, T, C.c_void_p(Yh.data_ptr()), st) == 1
    assert lib.moihgp_unproject_stream_tiled(gp.handle, 1, op, T, None, st) == 1
    assert lib.moihgp_unproject_stream_tiled(gp.handle, 1, C.c_void_p(out.data_ptr() + 4), T, C.c_void_p(Yh.data_ptr()), st) == 1
    assert lib.moihgp_unproject_stream_tiled(gp.handle, 1, op, 0, C.c_void_p(Yh.data_ptr()), st) == 0
    bank = S.LatentBank(0.1, _igp_params(L, np.random.default_rng(4)), kernel="Matern32")          # latents only: no mixing to project with
    assert lib.moihgp_project_stream_tiled(bank._h, 1, yp, T, op, st) == 1
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((Yh == SENTINEL).all())
    # T == 0 through Python
    e = S.project_stream_tiled(gp, Y[:0])
    assert tuple(e.shape) == (0, L, seg) and tuple(S.unproject_stream_tiled(gp, e, 0).shape) == (0, M)


@pytest.mark.gpu
@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("tiled", [0, 1])
def test_cxx_predict_stream_matches_python(env, hip_built, kern, tiled):
    """MOIHGPRegression::predictStream against filter_outputs with the same layout, 2 % of the outputs missing: the bar of
    test_cxx_predict_smoothed_matches_python."""
    torch, S = env["torch"], env["streams"]
    rng = np.random.default_rng(10)
    M, L, T = 12, 4, 300
    params = np.concatenate([(np.eye(M, L) + 0.2 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.05], _igp_params(L, rng).ravel()])
    Y = np.sin(0.02 * np.arange(T)[:, None] * (1 + np.arange(M)[None, :] % 5)) + 0.1 * rng.standard_normal((T, M))
    Y[rng.random((T, M)) < 0.02] = np.nan
    fmt = lambda a: " ".join("nan" if np.isnan(v) else repr(float(v)) for v in np.ravel(a))
    inp = f"{0 if kern == 'Matern32' else 1} {M} {L} 0.1 {T} {tiled}\n{fmt(params)}\n" + "\n".join(fmt(y) for y in Y) + "\n"
    out = subprocess.run([cxx_test_binary(hip_built, "predict_stream_test")], input=inp, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    got = np.array([[float(v) for v in line.split()] for line in out])
    gp = env["MOIHGP"](0.1, M, L, kernel=KMAP[kern])
    gp.update(params)
    Yh, _, _ = S.filter_outputs(gp, torch.from_numpy(Y).cuda(), layout="tiled" if tiled else "series")
    torch.cuda.synchronize()
    assert got.shape == (T, M) and np.isfinite(got).all()
    assert rel_err(got, Yh.cpu().numpy()) <= 1e-12
