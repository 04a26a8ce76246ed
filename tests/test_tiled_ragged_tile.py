"""GPU suite (-m gpu): the ragged last tile of a segment-major stream in the many-latent filter sweep (filter_dma_kernel TILED,
csrc/recursion.hip).  A tile is 4 KB of ticks (1024 fp32 / 512 fp64), a piece a quarter of it; the last tile of a stream whose length is
no multiple of the tile is allocated whole, but the sweep moves only its 16-byte vectors that hold a tick of the stream: the DMA lanes past
the end re-read the last such vector, and result vectors past the end are not stored.  None of that may change a result: every case against
the oracle, bit for bit against the series-major sweep of the same stream, with the input's padding holding zeros, NaN and 1e30 in turn,
and with the output pre-filled with a sentinel that must be gone below T and must survive in every vector of the last tile past it."""
import numpy as np
import pytest
import torch

from conftest import rel_err, rel_err_rows
from parity_support import FP32_TOL, FP64_TIGHT, KMAP, env, synth, synth_params, to_dev  # noqa: F401  (env: fixture)

pytestmark = pytest.mark.gpu

SEG = {torch.float32: 1024, torch.float64: 512}              # ticks per tile; a piece is a quarter of it, a vector 16 bytes
SENTINEL = {torch.float32: (torch.int32, np.uint32, 0x5A5AC3C3), torch.float64: (torch.int64, np.uint64, 0x5A5AC3C3A5A53C3C)}


def _lengths(dtype):
    """Stream lengths around the ragged tile: one tile plus 1 tick, a piece less a tick, exactly a piece, a piece and a tick, three pieces,
    three pieces and a tick, a tile less a tick, exactly two tiles; a single ragged tile shorter than the ring's first piece; and four
    tiles plus 784 ticks, whose refills run unclamped, clamped and not at all."""
    s = SEG[dtype]; p = s // 4
    return [s + 1, s + p - 1, s + p, s + p + 1, s + 3 * p, s + 3 * p + 1, 2 * s - 1, 2 * s, 16, 4 * s + 784]


CASES = [(dtype, T) for dtype in (torch.float64, torch.float32) for T in _lengths(dtype)]
IDS = [f"{'f64' if d == torch.float64 else 'f32'}-T{T}" for d, T in CASES]
# a gap among the valid ticks of the ragged tile (one tile + three pieces + 1 tick)
GAP_CASES = [(dtype, SEG[dtype] + 3 * (SEG[dtype] // 4) + 1) for dtype in (torch.float64, torch.float32)]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _ragged_tile(env, kern, dtype, L, T, gap):
    S, cref = env["streams"], env["cref"]
    seg, epv = SEG[dtype], 16 // (8 if dtype == torch.float64 else 4)
    nseg = (T + seg - 1) // seg
    tlast = T - (nseg - 1) * seg                              # ticks of the stream in its last tile
    rng = np.random.default_rng(31 * L + T)
    prm = synth_params(L, rng)
    Ty = synth(L, T, rng)
    x0 = 0.2 * rng.standard_normal((L, 2 if kern == "Matern32" else 3))
    if gap:
        Ty[::3, (nseg - 1) * seg + min(5, tlast - 1)] = np.nan      # inside the ragged tile, below T: its segment takes the missing-data path
    o = cref.filter_stream(cref.ihgp_array(kern, 0.1, prm), Ty, x0=x0, nthreads=8)
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6            # (the literal DARE leaves a few draws unstable)
    print(f"{kern} L={L} T={T}: {int(tame.sum())} of {L} latents tame; last tile holds {tlast} of {seg} ticks")
    assert tame.sum() >= 0.97 * L
    bank = S.LatentBank(0.1, prm, kernel=KMAP[kern])
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    Tyd = to_dev(Ty, dtype)
    xd = torch.from_numpy(x0).to(dtype).cuda()
    ity, inp, sent = SENTINEL[dtype]

    def tiled_run(pad):
        """The segment-major sweep with the input's padding ticks set to `pad` and the output pre-filled with the sentinel."""
        Tt = S.tile_stream(Tyd, T)
        assert tuple(Tt.shape) == (nseg, L, seg)
        Tt[-1, :, tlast:] = pad
        yt = torch.empty_like(Tt)
        yt.view(ity).fill_(sent)
        tot = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        _, xb, nb = bank.filter_tiled(Tt, T, x=xd.clone(), yhat=yt, nll_total=tot)
        torch.cuda.synchronize()
        return yt, (S.untile_stream(yt, T)[:, :T].cpu().numpy(), xb.cpu().numpy(), nb.cpu().numpy(), tot.cpu().numpy())

    tot_s = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    yhat, xT, nll = bank.filter(Tyd, T=T, x=xd.clone(), nll_total=tot_s)
    torch.cuda.synchronize()
    series = (yhat[:, :T].cpu().numpy(), xT.cpu().numpy(), nll.cpu().numpy(), tot_s.cpu().numpy())
    yt, tiled = tiled_run(0.0)

    # (a) against the oracle, both layouts
    for name, (yh, xs, nl, _) in (("series", series), ("tiled", tiled)):
        e = (rel_err_rows(np.nan_to_num(yh[tame]), np.nan_to_num(o["yhat"][tame])), rel_err(xs[tame], o["x"][tame]),
             rel_err(nl[tame], o["nll_per_latent"][tame]))
        print(f"  {name}: rel err yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e} (tol {tol:.0e})")
        assert max(e) < tol, (name, e)
    # (b) bit-equal to series-major (series-major Matern-5/2 at up to 1024 latents may take the eight-wavefront team kernel instead)
    if kern == "Matern32" or L > 1024:
        for what, a, b in zip(("yhat", "x", "nll", "nll_total"), series, tiled):
            assert _bits(a) == _bits(b), f"tiled {what} differs from series-major"
    # (d) the output's padding: no sentinel below T; every vector of the last tile without a tick below T keeps it
    assert not (np.ascontiguousarray(tiled[0]).view(inp) == inp(sent)).any(), "a result tick below T was not written"
    dead = (tlast + epv - 1) // epv * epv                     # first tick of the first vector that holds no tick of the stream
    kept = yt[-1, :, dead:].contiguous().view(ity).cpu().numpy().view(inp)
    print(f"  last tile: {(seg - dead) // epv} of {seg // epv} vectors per latent past the end, "
          f"{int((kept != inp(sent)).sum())} of their {kept.size} words overwritten")
    assert (kept == inp(sent)).all(), "the sweep stored a result vector that holds no tick of the stream"
    if gap:
        return
    # (c) the input's padding is ignored
    for pad in (float("nan"), 1e30):
        _, other = tiled_run(pad)
        for what, a, b in zip(("yhat", "x", "nll", "nll_total"), tiled, other):
            assert _bits(a) == _bits(b), f"{what} depends on the input's padding ({pad})"


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("L", [513, 1029])
@pytest.mark.parametrize("dtype,T", CASES, ids=IDS)
def test_ragged_last_tile(env, kern, L, dtype, T):
    """Every length at which the count of live vectors, pieces and clamped refills of the last tile changes, from a non-zero start state:
    oracle, series-major bit for bit, input padding ignored, output padding untouched."""
    _ragged_tile(env, kern, dtype, L, T, gap=False)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype,T", GAP_CASES, ids=["f64", "f32"])
def test_gap_in_ragged_tile(env, kern, dtype, T):
    """A NaN among the valid ticks of the ragged tile of every third latent: that segment leaves the fast path for generic_segment and its
    results leave through the same masked stores."""
    _ragged_tile(env, kern, dtype, 1029, T, gap=True)
