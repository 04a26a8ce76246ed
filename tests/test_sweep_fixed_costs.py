"""GPU suite (-m gpu): the fixed costs of the many-latent filter sweep (filter_dma_kernel / nll_total_kernel, csrc/recursion.hip) --
the refills of the LDS ring walk running addresses with the four pieces of a tile told apart by the instruction's offset, rows 1 and 2 of
the fp32 segment solve are packed pairs, and the NLL total batches its loads.  None of that may change a result: the sweep against the
oracle at the ring's boundaries (a ring is NP = 8 pieces of 256 fp32 / 128 fp64 ticks, a segment four of them), with the missing-data
path taken in segment 0 right behind the prologue's wait, and the total against its own fixed summation order, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err, rel_err_rows
from parity_support import FP32_TOL, FP64_TIGHT, KMAP, env, synth, synth_params, to_dev  # noqa: F401  (env: fixture)

pytestmark = pytest.mark.gpu

# stream lengths around the ring: less than / exactly / just past one piece count each -- one piece, a ragged fourth piece, five pieces less
# a tick, the whole ring less a tick (fp32) / two rings (fp64), exactly, one tick more, a ring and a half plus a tick, two rings exactly
RING_CASES = [(513, 256), (514, 1023), (516, 1279), (513, 2047), (515, 2048), (517, 2049), (1027, 3073), (518, 4096)]
# beyond the issue's list: more than 1024 latents, so that series-major Matern-5/2 takes this kernel too, and five fp32 segments, so that its
# refills run unclamped, clamped and not at all
RING_CASES.append((1029, 4097))
NAN_CASES = [(513, 2048), (1027, 3073)]


@functools.lru_cache(maxsize=None)
def _case(kern, L, T, gaps):
    """Inputs and the oracle's answer of one case: computed once, shared by both precisions, never written to."""
    from oracle import cref
    rng = np.random.default_rng(31 * L + T)
    prm = synth_params(L, rng)
    Ty = synth(L, T, rng)
    x0 = 0.2 * rng.standard_normal((L, 2 if kern == "Matern32" else 3))
    if gaps:
        Ty[::3, 0] = np.nan              # tick 0 of every third latent: segment 0 goes down the missing-data path
        Ty[L // 2, :] = np.nan           # one latent without a single observation
    o = cref.filter_stream(cref.ihgp_array(kern, 0.1, prm), Ty, x0=x0, nthreads=8)
    tame = np.nan_to_num(np.abs(o["yhat"]), nan=0.0).max(axis=1) < 1e6            # (the literal DARE leaves a few draws unstable)
    for a in (prm, Ty, x0, tame, o["yhat"], o["x"], o["nll_per_latent"]):
        a.setflags(write=False)
    return prm, Ty, x0, o, tame


def _sweep_both_layouts(env, kern, dtype, L, T, gaps):
    S = env["streams"]
    prm, Ty, x0, o, tame = _case(kern, L, T, gaps)
    print(f"{kern} L={L} T={T}: {int(tame.sum())} of {L} latents tame")
    assert tame.sum() >= 0.97 * L
    bank = S.LatentBank(0.1, prm, kernel=KMAP[kern])
    tol = FP64_TIGHT if dtype == torch.float64 else FP32_TOL
    Tyd = to_dev(Ty, dtype)
    xd = torch.from_numpy(x0).to(dtype).cuda()
    yhat, xT, nll = bank.filter(Tyd, T=T, x=xd.clone())
    yt, xb, nb = bank.filter_tiled(S.tile_stream(Tyd, T), T, x=xd.clone())
    torch.cuda.synchronize()
    got, got_t = yhat[:, :T].cpu().numpy(), S.untile_stream(yt, T)[:, :T].cpu().numpy()
    res = {"series": (got, xT.cpu().numpy(), nll.cpu().numpy()), "tiled": (got_t, xb.cpu().numpy(), nb.cpu().numpy())}
    for name, (yh, xs, nl) in res.items():
        e = (rel_err_rows(np.nan_to_num(yh[tame]), np.nan_to_num(o["yhat"][tame])), rel_err(xs[tame], o["x"][tame]),
             rel_err(nl[tame], o["nll_per_latent"][tame]))
        print(f"  {name}: rel err yhat {e[0]:.2e} x {e[1]:.2e} nll {e[2]:.2e} (tol {tol:.0e})")
        assert max(e) < tol, (name, e)
    if gaps:
        assert res["series"][2][L // 2] == 0.0 and res["tiled"][2][L // 2] == 0.0      # no observation, no NLL term
    # series-major Matern-5/2 at up to 1024 latents may take the eight-wavefront team kernel instead: the same kernel otherwise
    if kern == "Matern32" or L > 1024:
        for a, b in zip(res["series"], res["tiled"]):
            assert np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T", RING_CASES)
def test_ring_boundaries_vs_oracle(env, kern, dtype, L, T):
    """Stream lengths at which the prologue's clamped pieces, the first counted wait and the first / last refill change: against the oracle
    on every tame latent from a non-zero start state, both layouts, and tiled == series-major bit for bit where the kernel is the same."""
    _sweep_both_layouts(env, kern, dtype, L, T, gaps=False)


@pytest.mark.parametrize("kern", ["Matern32", "Matern52"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,T", NAN_CASES)
def test_constants_used_at_once(env, kern, dtype, L, T):
    """A gap at tick 0: segment 0 leaves the fast path at its first vote and runs generic_segment, which reads the constant block and the
    ring through ordinary loads, immediately behind the prologue's wait for the per-lane constants and the ring's head; one latent has no
    observation at all."""
    _sweep_both_layouts(env, kern, dtype, L, T, gaps=True)


def _total_in_kernel_order(nll):
    """nll_total_kernel's summation, re-enacted: 1024 threads add their strided terms in order, every 64 lanes fold by the xor butterfly
    32 .. 1, thread 0 adds the 16 wavefront sums in order."""
    s = np.zeros(1024, dtype=np.float64)
    for b in range(0, len(nll), 1024):
        part = nll[b:b + 1024]
        s[:len(part)] = s[:len(part)] + part
    w = s.reshape(16, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lanes ^ o]
    t = np.float64(0.0)
    for k in range(16):
        t = t + w[k, 0]
    return t


@pytest.mark.parametrize("L", [513, 1024, 1025, 4096, 8193, 9001])
def test_nll_total_fixed_order(env, L):
    """Less than one pass of the 1024 threads, exactly one, one term more, one full batch of loads, one term past a batch, a ragged second
    batch: the total equals the fixed-order sum of the returned per-latent terms bit for bit."""
    S = env["streams"]
    T = 40
    rng = np.random.default_rng(31 * L + T)
    bank = S.LatentBank(0.1, synth_params(L, rng), kernel="Matern52ss")
    Tyd = to_dev(synth(L, T, rng), torch.float32)
    total = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    _, _, nll = bank.filter(Tyd, T=T, want_yhat=False, nll_total=total)
    torch.cuda.synchronize()
    nl = nll.cpu().numpy()
    got, exp = total.cpu().numpy()[0], _total_in_kernel_order(nl)
    print(f"L={L}: total {got!r}, re-enacted {exp!r}, plain sum {nl.sum()!r}")
    assert np.isfinite(nl).all()
    assert got.tobytes() == exp.tobytes()
