"""The MFMA dense products (csrc/gemm_mfma.hip) through the public ABI, at tile, k-slab and alignment edges.

    projection     Ty[l][t]   = S_l^-1/2 sum_m U[m][l] Y[t][m]            i = l < L, j = t < T, k = m < M
    un-projection  Yhat[t][m] = sum_l Tyhat[l][t] S_l^1/2 U[m][l]          i = t < T, j = m < M, k = l < L

The mixing is installed with moihgp_set_mixing (any U and S, one upload, no polar factor); the products are moihgp_project_stream,
moihgp_unproject_stream and their _tiled forms, called through ctypes wherever a test sets the pointer or the leading dimension.

 1. Exact products.  Small integers in U and the streams and S_l in {1/4, 1, 4, 16}: the square roots are powers of two and every product
    and partial sum is a multiple of 1/2 below 24 K < 2^23, so the fp32 and the fp64 kernels must return the float64 numpy product exactly,
    whatever their summation order -- np.array_equal, no tolerance.  S differs from latent to latent, so a row scale or a k scale read at
    the wrong index is a mismatch.  Every output starts as NaN inside a larger allocation filled with a bit pattern that must survive; every
    input lies in NaN, so a fetch outside its payload poisons the result.
 2. Rounding.  Real inputs, S log-uniform in [1e-4, 1e4]: every entry within (K + 8) u scale of a long-double reference of the values the
    device is given, scale = the entry's own sum of absolute terms (BAR below).
 3. The fp32 image of the mixing follows every route that changes U.
 4. The triangular Gram launch behind moihgp_set_mixing, tile by tile, through the switch it feeds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from parity_support import env, synth_params  # noqa: F401  (env: fixture)

pytestmark = pytest.mark.gpu

DTYPES = {"fp64": torch.float64, "fp32": torch.float32}
FRONT = 64                                              # elements in front of and behind a payload: a multiple of 16 bytes in both types
SENTINEL = {8: 0x5AA55AA55AA55AA5, 4: 0x5AA55AA5}        # (finite numbers in both types; compared as integers)
KSET = [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65]  # k depths around the slabs of 16 and the tiles of 32

_HANDLES = {}       # (M, L) -> [gp, tag of the installed mixing]
_EXACT = {}         # (M, L, T) -> the integer case and its float64 products
_REAL = {}          # (M, L, T, S draw, dtype) -> the real case, its long-double products and their bars


# ------------------------------------------------------------------------------------------------ device buffers
def _int_dtype(dtype):
    return (torch.int64, np.int64) if dtype == torch.float64 else (torch.int32, np.int32)


class Region:
    """A rows x cols payload with leading dimension ld, `off` elements past a 16-byte aligned address inside a larger allocation: the payload
    holds NaN, everything else -- in front, behind and between the rows -- the sentinel bit pattern."""

    def __init__(self, dtype, rows, cols, ld, off=0):
        self.dtype, self.rows, self.cols, self.ld = dtype, rows, cols, ld
        self.size = dtype.itemsize
        self.start = FRONT + off
        self.empty = rows == 0 or cols == 0
        span = 0 if self.empty else (rows - 1) * ld + cols
        self.n = self.start + span + FRONT
        tint, nint = _int_dtype(dtype)
        self.raw = torch.from_numpy(np.full(self.n, SENTINEL[self.size], dtype=nint)).cuda()
        assert self.raw.data_ptr() % 16 == 0
        self.val = self.raw.view(dtype)
        if not self.empty:
            torch.as_strided(self.val, (rows, cols), (ld, 1), self.start).fill_(float("nan"))
        self.ptr = C.c_void_p(self.raw.data_ptr() + self.start * self.size)

    def read(self):
        """(payload [rows, cols] as float64, True if nothing outside the payload has changed)."""
        raw = self.raw.cpu().numpy()
        outside = np.ones(self.n, dtype=bool)
        if self.empty:
            return np.zeros((self.rows, self.cols)), bool((raw == SENTINEL[self.size]).all())
        idx = self.start + np.arange(self.rows)[:, None] * self.ld + np.arange(self.cols)[None, :]
        outside[idx.ravel()] = False
        vals = raw.view(np.float64 if self.size == 8 else np.float32)
        return vals[idx].astype(np.float64), bool((raw[outside] == SENTINEL[self.size]).all())


def _operand(a, dtype, ld=None, off=0):
    """(tensor that owns the memory, pointer) of the input a [rows, cols] with leading dimension ld, `off` elements past a 16-byte aligned address;
    NaN everywhere outside the payload."""
    rows, cols = a.shape
    ld = cols if ld is None else ld
    start = FRONT + off
    n = start + (0 if rows == 0 or cols == 0 else (rows - 1) * ld + cols) + FRONT
    buf = torch.full((n,), float("nan"), dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if rows and cols:
        torch.as_strided(buf, (rows, cols), (ld, 1), start).copy_(torch.from_numpy(np.array(a)).to(dtype))      # (np.array: a writable copy)
    return buf, C.c_void_p(buf.data_ptr() + start * dtype.itemsize)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(dtype):
    return 0 if dtype == torch.float64 else 1


# ------------------------------------------------------------------------------------------------ handles and mixings
def _handle(env, M, L):
    if (M, L) not in _HANDLES:
        _HANDLES[(M, L)] = [env["MOIHGP"](0.1, M, L, kernel="Matern32"), None]
    return _HANDLES[(M, L)]


def _set_mixing(env, gp, U, S, sigma=0.05):
    from multioutputihgp_amd._lib import c_double_p
    U = np.ascontiguousarray(U, dtype=np.float64); S = np.ascontiguousarray(S, dtype=np.float64)
    assert env["lib"].moihgp_set_mixing(gp.handle, U.ctypes.data_as(c_double_p), S.ctypes.data_as(c_double_p), C.c_double(sigma)) == 0


def _with_mixing(env, M, L, tag, U, S):
    """The shared handle of (M, L) with the mixing `tag` installed (one upload per change of tag)."""
    h = _handle(env, M, L)
    if h[1] != tag:
        _set_mixing(env, h[0], U, S)
        h[1] = tag
    return h[0]


# ------------------------------------------------------------------------------------------------ the two products through ctypes
def _project(env, gp, dtype, Y, L, ld=None, off_in=0, off_out=0):
    """moihgp_project_stream of Y [T, M] at `off_in` elements past an aligned address into a guarded [L][ld] buffer at `off_out`:
    (Ty [L, T] float64, guard intact)."""
    T = Y.shape[0]
    ld = T if ld is None else ld
    keep, yptr = _operand(Y, dtype, off=off_in)
    out = Region(dtype, L, T, ld, off_out)
    rc = env["lib"].moihgp_project_stream(gp.handle, _dt(dtype), yptr, T, out.ptr, ld, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.read()


def _unproject(env, gp, dtype, Tyhat, M, ld=None, off_in=0, off_out=0):
    """moihgp_unproject_stream of Tyhat [L, T] with leading dimension ld at `off_in` into a guarded [T][M] buffer at `off_out`:
    (Yhat [T, M] float64, guard intact)."""
    T = Tyhat.shape[1]
    ld = T if ld is None else ld
    keep, tptr = _operand(Tyhat, dtype, ld=ld, off=off_in)
    out = Region(dtype, T, M, M, off_out)
    rc = env["lib"].moihgp_unproject_stream(gp.handle, _dt(dtype), tptr, T, ld, out.ptr, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.read()


def _project_tiled(env, gp, dtype, Y, L):
    """moihgp_project_stream_tiled into [nseg][L][SEG] between two guards: NaN in the ticks < T, the sentinel in the spare ticks of the last tile.
    (Ty [L, T] float64, True if the spare ticks and the guards are unchanged)."""
    T = Y.shape[0]
    seg = env["streams"].seg_ticks(dtype)
    nseg = (T + seg - 1) // seg
    size = dtype.itemsize
    tint, nint = _int_dtype(dtype)
    raw = torch.from_numpy(np.full(2 * FRONT + nseg * L * seg, SENTINEL[size], dtype=nint)).cuda()
    tiles = raw.view(dtype)[FRONT:FRONT + nseg * L * seg].view(nseg, L, seg)
    for s in range(nseg):
        tiles[s, :, :min(seg, T - s * seg)] = float("nan")
    keep, yptr = _operand(Y, dtype)
    rc = env["lib"].moihgp_project_stream_tiled(gp.handle, _dt(dtype), yptr, T, C.c_void_p(tiles.data_ptr()), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    h = raw.cpu().numpy()
    body = h[FRONT:FRONT + nseg * L * seg].reshape(nseg, L, seg).transpose(1, 0, 2).reshape(L, nseg * seg)
    intact = bool((h[:FRONT] == SENTINEL[size]).all() and (h[-FRONT:] == SENTINEL[size]).all() and (body[:, T:] == SENTINEL[size]).all())
    return np.ascontiguousarray(body[:, :T]).view(np.float64 if size == 8 else np.float32).astype(np.float64), intact


def _unproject_tiled(env, gp, dtype, Tyhat, M):
    """moihgp_unproject_stream_tiled of Tyhat [L, T] laid out [nseg][L][SEG] with NaN in the ticks >= T of the last tile."""
    L, T = Tyhat.shape
    seg = env["streams"].seg_ticks(dtype)
    nseg = (T + seg - 1) // seg
    full = np.full((L, nseg * seg), np.nan)
    full[:, :T] = Tyhat
    tiles = torch.from_numpy(np.ascontiguousarray(full.reshape(L, nseg, seg).transpose(1, 0, 2))).to(dtype).cuda()
    assert tiles.data_ptr() % 16 == 0
    out = Region(dtype, T, M, M)
    rc = env["lib"].moihgp_unproject_stream_tiled(gp.handle, _dt(dtype), C.c_void_p(tiles.data_ptr()), T, out.ptr, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.read()


# ================================================================================================ 1. exact products
def _exact_case(M, L, T):
    """Integer inputs and their products in float64 (exact: every term and partial sum is a multiple of 1/2 below 2^23)."""
    key = (M, L, T)
    if key not in _EXACT:
        rng = np.random.default_rng([M, L, T])
        U = rng.integers(-2, 3, (M, L)).astype(np.float64)
        S = rng.choice([0.25, 1.0, 4.0, 16.0], L)
        Y = rng.integers(-3, 4, (T, M)).astype(np.float64)
        Tyhat = rng.integers(-3, 4, (L, T)).astype(np.float64)
        ty = ((Y @ U) / np.sqrt(S)).T
        yhat = (Tyhat.T * np.sqrt(S)) @ U.T
        for a in (U, S, Y, Tyhat, ty, yhat):
            a.setflags(write=False)
        _EXACT[key] = dict(U=U, S=S, Y=Y, Tyhat=Tyhat, ty=ty, yhat=yhat)
    return _EXACT[key]


def _exact_gp(env, M, L, T):
    c = _exact_case(M, L, T)
    return c, _with_mixing(env, M, L, ("exact", T), c["U"], c["S"])


def _assert_both_exact(env, dtype, M, L, T):
    c, gp = _exact_gp(env, M, L, T)
    ty, intact = _project(env, gp, dtype, c["Y"], L)
    assert intact, "the projection stored outside its [L][T] payload"
    assert np.array_equal(ty, c["ty"]), ("projection", _mismatch(ty, c["ty"]))
    yhat, intact = _unproject(env, gp, dtype, c["Tyhat"], M)
    assert intact, "the un-projection stored outside its [T][M] payload"
    assert np.array_equal(yhat, c["yhat"]), ("un-projection", _mismatch(yhat, c["yhat"]))


def _mismatch(got, want):
    """Where two arrays differ: the count, the first index, both values there and the number of entries never stored."""
    bad = np.argwhere(~(got == want))
    if not len(bad):
        return None
    i = tuple(int(v) for v in bad[0])
    return dict(count=len(bad), of=got.size, first=i, got=float(got[i]), want=float(want[i]), never_stored=int(np.isnan(got).sum()))


EXACT_SHAPES = ([(2, 1, 1), (3, 1, 1), (5, 5, 1)]                                             # degenerate
                + [(m, 8, 9) for m in KSET]                                                    # k depth of the projection
                + [(k + 1, k, 9) for k in KSET]                                                # k depth of the un-projection
                + [(m, l, t) for (m, l) in ((130, 127), (130, 128), (132, 129)) for t in (127, 128, 129, 257)]      # tile edges
                + [(260, 256, 130), (261, 256, 130), (262, 258, 130), (263, 257, 130)]         # vector and scalar fetches: L, M mod 4
                + [(1030, 1025, 129), (129, 8, 1100)])                                         # tile order: 9 x 2 tiles in either product


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("M,L,T", EXACT_SHAPES)
def test_exact_products(env, dt, M, L, T):
    """Both products of integer inputs equal the float64 numpy products exactly, nothing is stored outside the payload, nothing is left NaN."""
    _assert_both_exact(env, DTYPES[dt], M, L, T)


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
def test_empty_stream_touches_nothing(env, dt):
    """T = 0: rc 0 from all four entries and not one byte stored."""
    dtype, (M, L) = DTYPES[dt], (9, 8)
    c, gp = _exact_gp(env, M, L, 0)
    assert c["Y"].shape == (0, M) and c["Tyhat"].shape == (L, 0)
    for got, intact in (_project(env, gp, dtype, c["Y"], L), _unproject(env, gp, dtype, c["Tyhat"], M),
                        _project_tiled(env, gp, dtype, c["Y"], L), _unproject_tiled(env, gp, dtype, c["Tyhat"], M)):
        assert intact and got.size == 0


def _misaligned_configs():
    """(dtype name, product, offset of the input, its ld - T, offset of the output, the output's ld - T): every element offset from a 16-byte
    aligned address that keeps natural alignment (1 in fp64; 1, 2, 3 in fp32)."""
    out = []
    for dt, offs in (("fp64", (1,)), ("fp32", (1, 2, 3))):
        for o in offs:
            out.append((dt, "project", o, 0, 0, 0))               # Y off its vector alignment
            out.append((dt, "unproject", o, 0, 0, 0))             # Tyhat off its vector alignment, even ld (T = 130)
            out.append((dt, "unproject", o, 1, 0, 0))             # ... and odd ld
        out.append((dt, "project", 0, 0, 1, 0))                   # the output one element off, ld == T
        out.append((dt, "unproject", 0, 0, 1, 0))
        out.append((dt, "project", 0, 0, 0, 1))                   # ld = T + 1 on an aligned base
        out.append((dt, "unproject", 0, 1, 0, 0))
    return out


@pytest.mark.parametrize("dt,product,off_in,dld_in,off_out,dld_out", _misaligned_configs())
def test_exact_products_of_misaligned_operands(env, dt, product, off_in, dld_in, off_out, dld_out):
    """The public entries take any pointer and any ld >= T: operands that are not 16-byte aligned, or whose rows are not, go through the scalar
    fetches and give the same exact product; a vector load of such an operand would read other elements (or the NaN around it)."""
    dtype, (M, L, T) = DTYPES[dt], (260, 256, 130)
    c, gp = _exact_gp(env, M, L, T)
    if product == "project":
        got, intact = _project(env, gp, dtype, c["Y"], L, ld=T + dld_out, off_in=off_in, off_out=off_out)
        want = c["ty"]
    else:
        got, intact = _unproject(env, gp, dtype, c["Tyhat"], M, ld=T + dld_in, off_in=off_in, off_out=off_out)
        want = c["yhat"]
    assert intact, "stored outside the payload"
    assert np.array_equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("M,L,extra", [(263, 257, 129), (130, 128, 0)])
def test_exact_products_segment_major(env, dt, M, L, extra):
    """The _tiled entries at T = SEG + 129 (a second, ragged segment; scalar fetches) and T = SEG (one whole segment; vector fetches): the exact
    products again.  The projection leaves the spare ticks of the last tile and both guards alone; the un-projection never reads the spare
    ticks, which hold NaN."""
    dtype = DTYPES[dt]
    T = env["streams"].seg_ticks(dtype) + extra
    c, gp = _exact_gp(env, M, L, T)
    ty, intact = _project_tiled(env, gp, dtype, c["Y"], L)
    assert intact, "the tiled projection stored into spare ticks or outside the stream"
    assert np.array_equal(ty, c["ty"]), ("projection", _mismatch(ty, c["ty"]))
    yhat, intact = _unproject_tiled(env, gp, dtype, c["Tyhat"], M)
    assert intact, "the tiled un-projection stored outside its [T][M] payload"
    assert np.array_equal(yhat, c["yhat"]), ("un-projection", _mismatch(yhat, c["yhat"]))


# ================================================================================================ 2. rounding, entry by entry
UNIT = {torch.float64: 2.0 ** -53, torch.float32: 2.0 ** -24}


def BAR(K, dtype, scale):
    """The componentwise bound of a length-K product summed in any order, |fl(sum) - sum| <= K u sum|terms| to first order, with 8 more roundings
    for what surrounds the sum: U narrowed to float32, the scale's square root, reciprocal and cast, the multiply by the scale."""
    return (K + 8) * UNIT[dtype] * scale


def _products_ld(U, S, Y, Tyhat):
    """Both products and their scales (each entry's sum of absolute terms): the values in long double, the scales in float64."""
    ld = np.longdouble
    rs, Ul = np.sqrt(S.astype(ld)), U.astype(ld)
    ty = ((Y.astype(ld) @ Ul) / rs).T
    yhat = (Tyhat.astype(ld).T * rs) @ Ul.T
    ty_scale = ((np.abs(Y) @ np.abs(U)) / np.sqrt(S)).T
    yhat_scale = (np.abs(Tyhat).T * np.sqrt(S)) @ np.abs(U).T
    return ty, yhat, ty_scale, yhat_scale


def _real_case(M, L, T, sdraw, dtype):
    """Real inputs as the device is given them (the streams rounded to `dtype`, U and S in float64) with their long-double products."""
    key = (M, L, T, sdraw, dtype)
    if key not in _REAL:
        rng = np.random.default_rng([M, L, T, len(sdraw)])
        U = rng.standard_normal((M, L))
        S = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), L)) if sdraw == "box" else rng.uniform(0.5, 2, L)
        npdt = np.float64 if dtype == torch.float64 else np.float32
        Y = rng.standard_normal((T, M)).astype(npdt).astype(np.float64)
        Tyhat = rng.standard_normal((L, T)).astype(npdt).astype(np.float64)
        ty, yhat, ty_scale, yhat_scale = _products_ld(U, S, Y, Tyhat)
        _REAL[key] = dict(U=U, S=S, Y=Y, Tyhat=Tyhat, ty=ty, yhat=yhat, ty_scale=ty_scale, yhat_scale=yhat_scale)
    return _REAL[key]


def _worst(got, want, bar):
    """Largest err / bar over the entries, and where."""
    ratio = np.abs(got.astype(np.longdouble) - want).astype(np.float64) / bar
    ratio[np.isnan(ratio)] = np.inf
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), tuple(int(v) for v in i)


def _assert_both_within_bar(env, gp, dtype, c, M, L, what=""):
    ty, intact = _project(env, gp, dtype, c["Y"], L)
    w_p, at_p = _worst(ty, c["ty"], BAR(M, dtype, c["ty_scale"]))
    yhat, intact2 = _unproject(env, gp, dtype, c["Tyhat"], M)
    w_u, at_u = _worst(yhat, c["yhat"], BAR(L, dtype, c["yhat_scale"]))
    print("dense products %s M=%d L=%d T=%d %s: worst err / bar projection %.4f at %s, un-projection %.4f at %s"
          % (what, M, L, c["Y"].shape[0], "fp64" if dtype == torch.float64 else "fp32", w_p, at_p, w_u, at_u))
    assert intact and intact2, "stored outside the payload"
    assert w_p <= 1.0, ("projection", what, w_p, at_p)
    assert w_u <= 1.0, ("un-projection", what, w_u, at_u)


@pytest.mark.parametrize("dt", ["fp64", "fp32"])
@pytest.mark.parametrize("M,L,T,sdraw", [(65, 33, 9, "box"), (132, 129, 257, "box"), (263, 257, 130, "box"), (1030, 1025, 129, "box"),
                                         (132, 129, 257, "near1")])
def test_products_round_within_the_componentwise_bound(env, dt, M, L, T, sdraw):
    """Every entry of both products within (K + 8) u of its own sum of absolute terms, with S over the learner's box [1e-4, 1e4] ("box") or in
    [0.5, 2] ("near1": every k then contributes visibly to the un-projection)."""
    dtype = DTYPES[dt]
    c = _real_case(M, L, T, sdraw, dtype)
    gp = _with_mixing(env, M, L, ("real", T, sdraw), c["U"], c["S"])
    _assert_both_within_bar(env, gp, dtype, c, M, L, sdraw)


# ================================================================================================ 3. the fp32 image of the mixing
def test_fp32_image_follows_every_change_of_the_mixing(env):
    """The fp32 products read an fp32 image of U that exists from the first fp32 call on.  After update, moihgp_update_dev, moihgp_set_mixing and
    moihgp_reseed_U the fp32 products of a fixed stream must be those of the mixing read back, to the bar of part 2: an image left behind is off
    by the whole change of U."""
    M, L, T, dtype = 40, 20, 33, torch.float32
    lib = env["lib"]
    rng = np.random.default_rng(4020)
    gp = env["MOIHGP"](0.1, M, L, kernel="Matern32")
    Y = rng.standard_normal((T, M)).astype(np.float32).astype(np.float64)
    Tyhat = rng.standard_normal((L, T)).astype(np.float32).astype(np.float64)

    def params():
        return np.concatenate([(np.eye(M, L) + 0.3 * rng.standard_normal((M, L))).ravel(), rng.uniform(0.5, 2, L), [0.03], synth_params(L, rng).ravel()])

    def check(route, U_before):
        p = gp.params.copy()
        U, S = p[:M * L].reshape(M, L), p[M * L:M * L + L]
        if U_before is not None:
            assert np.max(np.abs(U - U_before)) > 1e-3, (route, "the route did not change U: the check would pass on a stale image")
        ty, yhat, ty_scale, yhat_scale = _products_ld(U, S, Y, Tyhat)
        c = dict(Y=Y, Tyhat=Tyhat, ty=ty, yhat=yhat, ty_scale=ty_scale, yhat_scale=yhat_scale)
        _assert_both_within_bar(env, gp, dtype, c, M, L, route)
        return U.copy()

    U0 = check("constructor", None)                          # the first fp32 products: the image exists from here on
    gp.update(params())
    U1 = check("update", U0)
    pd = torch.from_numpy(params()).cuda()
    torch.cuda.synchronize()
    assert lib.moihgp_update_dev(gp.handle, C.c_void_p(pd.data_ptr())) == 0
    U2 = check("moihgp_update_dev", U1)
    _set_mixing(env, gp, rng.standard_normal((M, L)), np.exp(rng.uniform(np.log(1e-4), np.log(1e4), L)))
    U3 = check("moihgp_set_mixing", U2)
    lib.moihgp_reseed_U(gp.handle, 12345)
    check("moihgp_reseed_U", U3)


# ================================================================================================ 4. the triangular Gram launch
def _tile_pair(tm, tn, L):
    """(a, b), a <= b: the entry G[a][b] at the corner of tile (tm, tn) of the upper triangle that lies farthest from the diagonal -- the first row
    of the tile and its last column.  a == b only where a diagonal tile holds a single entry."""
    return tm * 128, min(tn * 128 + 127, L - 1)


def _gram_pairs(L, tiles):
    return [_tile_pair(tm, tn, L) for tm, tn in tiles]


def _tiles_257():
    return [(tm, tn) for tm in range(3) for tn in range(tm, 3)]


def _tiles_1100():
    rng = np.random.default_rng(1100)
    upper = [(tm, tn) for tm in range(9) for tn in range(tm, 9)]
    fixed = [(0, 0), (0, 8), (7, 8), (8, 8), (3, 5)]
    rest = [t for t in upper if t not in fixed]
    return fixed + [rest[i] for i in rng.choice(len(rest), 5, replace=False)]


@pytest.mark.parametrize("L,tiles", [(257, _tiles_257()), (1100, _tiles_1100())], ids=["L257", "L1100"])
def test_gram_of_set_mixing_tile_by_tile(env, L, tiles):
    """moihgp_set_mixing forms U^T U with the symmetric launch into a work buffer that persists, and switches the least-squares projection of
    partially observed ticks on only if max|G - I| < 1e-9.  Q orthonormal: the tick with one NaN output projects to a finite column.  Q with
    column b += 1e-6 column a: G[a][b] = 1e-6 and the column is all NaN (a == b, where a diagonal tile holds one entry: column a scaled by
    1 + 1e-6, G[a][a] = 1 + 2e-6).  The two alternate, one probed tile after the other: a tile the launch skips keeps what the previous call
    left there, and the switch comes out wrong."""
    M = L + 2
    S_, rng = env["streams"], np.random.default_rng(L)
    Q, _ = np.linalg.qr(rng.standard_normal((M, L)))
    Q = np.ascontiguousarray(Q)
    assert np.max(np.abs(Q.T @ Q - np.eye(L))) < 1e-12
    Sv = rng.uniform(0.5, 2, L)
    y = rng.standard_normal((1, M)); y[0, M // 3] = np.nan
    Yd = torch.from_numpy(y).cuda()
    gp = _handle(env, M, L)
    gp[1] = ("gram",)
    gp = gp[0]

    def column(U):
        _set_mixing(env, gp, U, Sv)
        col = S_.project_stream(gp, Yd)[:, 0].cpu().numpy()
        return col

    assert np.isfinite(column(Q)).all()
    pairs = _gram_pairs(L, tiles)
    assert len(set(pairs)) == len(pairs)
    for (tm, tn), (a, b) in zip(tiles, pairs):
        assert a // 128 == tm and b // 128 == tn and a <= b
        Qp = Q.copy()
        if a == b:
            Qp[:, a] *= 1 + 1e-6
        else:
            Qp[:, b] += 1e-6 * Q[:, a]
        col = column(Qp)
        assert np.isnan(col).all(), ("tile", (tm, tn), "G[%d][%d] = 1e-6 went unseen" % (a, b), int(np.isnan(col).sum()))
        col = column(Q)
        assert np.isfinite(col).all(), ("tile", (tm, tn), "G[%d][%d] kept the defect of the previous call" % (a, b), int(np.isnan(col).sum()))
