"""CPU self-check that the loss / PSNR / SSIM GPU tests are sharp.

The GPU tests compare the kernels with the fp64 references of
tests/metrics_ref.py at the tolerances stated there.  Here the same input
builders and the same tolerances are taken, the defects a kernel of this kind
can have are applied to the fp64 restatement itself (never to a tolerance),
and each must move the result by more than the GPU test allows -- for every
shape and value range the GPU test runs, and for every sample the defect
touches:
  SSIM   the last input column / row / depth slice read as zeros (a halo that
         was not loaded; on the 17611-row image, where the image's last row
         reaches one output in 17601, the last halo row of every tile); the
         output columns x = 32 k and rows y = 16 k, where the 16 x 32 tiles
         meet, replaced by their neighbours; the per-sample sum stopping at
         1024 tiles; two samples' maps of one channel exchanged; an output
         depth computed from its neighbour's moment planes
  loss   the tail element dropped; an element at a lap boundary counted twice
  PSNR   every localised place (first, last, both sides of every chunk
         boundary) dropped, and counted twice; round-half-away instead of
         half-to-even on the exact-tie inputs
"""
import pytest
import torch

from tests import metrics_ref as R

IDS2D = ["x".join(map(str, s)) for s in R.SSIM2D_SHAPES]
IDS3D = ["x".join(map(str, s)) for s in R.SSIM3D_SHAPES]


def _ranges(shape):
    c, dim = R.ssim_case(shape), len(shape) - 2
    yield "255", c.o255.double(), c.t255.double(), 255.0, c.ref255, R.ssim_tol(dim, 255)
    yield "1", c.o1.double(), c.t1.double(), 1.0, c.ref1, R.ssim_tol(dim, 1)


def _caught(tag, ref, mutant, tol, samples=None):
    moved = (mutant - ref).abs()
    if samples is not None:
        moved = moved[samples]
    assert bool((moved > tol).all()), (tag, moved.tolist(), tol)


def _zero_edge(x, axis):
    x = x.clone()
    x.select(axis, x.shape[axis] - 1).zero_()
    return x


def _seam(m, axis, step):
    """The first output line of every tile but the first takes its neighbour's value."""
    at = torch.arange(step, m.shape[axis], step)
    return m.index_copy(axis, at, m.index_select(axis, at - 1))


@pytest.mark.parametrize("shape", R.SSIM2D_SHAPES + R.SSIM3D_SHAPES, ids=IDS2D + IDS3D)
def test_ssim_mutants_are_caught(shape):
    n, ch, *sp = shape
    for tag, o, t, vr, ref, tol in _ranges(shape):
        m = R.ssim_map(o, t, vr)
        assert torch.equal(R.per_sample(m), ref)
        # a halo that was not loaded, on each spatial axis
        for axis in range(2, len(shape)):
            if len(sp) == 2 and axis == 2 and m.shape[2] > 1024:
                # the image's last row reaches one output in 17601 here (and
                # with the window's 1 % edge weight): the other shapes hold
                # that defect.  What this shape holds is the same defect per
                # tile: the last halo row of every 16-row tile read as zeros,
                # i.e. outputs y = 16 k + 15 computed without input row y + 10.
                rows = torch.arange(R.SSIM_TY - 1, m.shape[2], R.SSIM_TY)
                oz, tz = o.clone(), t.clone()
                oz[:, :, rows + R.SSIM_WIN - 1] = 0
                tz[:, :, rows + R.SSIM_WIN - 1] = 0
                mut = m.clone()
                mut[:, :, rows] = R.ssim_map(oz, tz, vr)[:, :, rows]
                _caught(f"{tag} zero tile halo row", ref, R.per_sample(mut), tol)
                continue
            mut = R.per_sample(R.ssim_map(_zero_edge(o, axis), _zero_edge(t, axis), vr))
            _caught(f"{tag} zero edge axis {axis}", ref, mut, tol)
        # tile seams
        if sp[-1] - R.SSIM_WIN + 1 > R.SSIM_TX:
            _caught(f"{tag} seam column", ref, R.per_sample(_seam(m, m.dim() - 1, R.SSIM_TX)), tol)
        if sp[-2] - R.SSIM_WIN + 1 > R.SSIM_TY:
            _caught(f"{tag} seam row", ref, R.per_sample(_seam(m, m.dim() - 2, R.SSIM_TY)), tol)
        # ssim_final stopping after one lap of its 1024 lanes (2-D, one tile per 16 rows)
        if len(sp) == 2 and -(-m.shape[-2] // R.SSIM_TY) * -(-m.shape[-1] // R.SSIM_TX) > 1024 and m.shape[-1] <= 32:
            cut = m.clone()
            cut[..., 1024 * R.SSIM_TY:, :] = 0
            _caught(f"{tag} one lap", ref, cut.flatten(1).sum(1) / m[0].numel(), tol)
        # one channel's maps exchanged between two samples
        if n > 1 and ch > 1:
            sw = m.clone()
            sw[0, 1], sw[1, 1] = m[1, 1], m[0, 1]
            _caught(f"{tag} channel swap", ref, R.per_sample(sw), tol, samples=[0, 1])
        # samples exchanged (what the permutation tests would see)
        if n > 1:
            assert bool((ref[0] - ref[1]).abs() > tol)


@pytest.mark.parametrize("shape", [(2, 2, 12, 28, 44), (1, 3, 13, 27, 43)], ids=["2x2x12x28x44", "1x3x13x27x43"])
def test_ssim3d_plane_mutants_are_caught(shape):
    """dout > 1: two output depths' planes exchanged within a volume change
    nothing in a mean, so the defect that matters is one output depth computed
    from the neighbouring depth's moments (img off by one in the moment planes)."""
    for tag, o, t, vr, ref, tol in _ranges(shape):
        m = R.ssim_map(o, t, vr)
        mut = m.clone()
        mut[:, :, 1] = m[:, :, 0]
        _caught(f"{tag} depth plane", ref, R.per_sample(mut), tol)


@pytest.mark.parametrize("count", R.LOSS_LOCALISED_COUNTS)
@pytest.mark.parametrize("spec", range(len(R.LOSS_SPECS)), ids=R.LOSS_SPEC_IDS)
def test_loss_mutants_are_caught(spec, count):
    c = R.loss_case(spec, count, True)
    terms = R.loss_terms(c.kind, R.f32(c.p), c.o.double() - c.t.double())
    assert terms.mean().item() == pytest.approx(c.loss, rel=1e-14)
    tol = R.loss_bound(c.loss)
    dropped = terms[:-1].sum().item() / count
    assert abs(dropped - c.loss) > tol, ("tail dropped", dropped, c.loss, tol)
    for i in c.idx:  # 256, 2^20, 2^21: where a block or a lap begins
        twice = (terms.sum() + terms[i]).item() / count
        assert abs(twice - c.loss) > tol, ("counted twice", i, twice, c.loss, tol)
    # the gradient: a lane that is never written keeps whatever was there; the
    # reference at the perturbed places is far from 0 relative to its bound
    b = R.grad_bound(c.grad[c.idx], torch.float16)
    assert bool((c.grad[c.idx].abs() > b).all())


@pytest.mark.parametrize("per", R.PSNR_LOCALISED_PER)
def test_psnr_mutants_are_caught(per):
    o, t, groups = R.psnr_localised(per)
    ref = R.psnr_ref(o, t)
    idx, pc = R.psnr_boundary_indices(per)
    assert sorted(i for g in groups for i in g) == idx and 0 in idx and per - 1 in idx
    assert all(k * pc in idx and k * pc - 1 in idx for k in range(1, R.PSNR_CHUNKS))
    d2 = (o.double() - t.double()) ** 2
    for b, grp in enumerate(groups):
        s = d2[b].sum()
        for i in grp:
            for what, s_mut in (("dropped", s - d2[b, i]), ("twice", s + d2[b, i])):
                mut = 10 * torch.log10(255.0 ** 2 / (s_mut / per + R.f32(1e-10)))
                assert abs(mut.item() - ref[b].item()) > R.PSNR_EXACT_TOL_DB, (what, b, i)


def test_psnr_round_half_away_is_caught():
    o, t, mean, std = R.psnr_ties()
    ref = R.psnr_ref(R.denorm64(o, mean, std), R.denorm64(t, mean, std))

    def away(x):
        v = x.double() * R.f32(std) + R.f32(mean)
        assert bool((v - torch.floor(v) == 0.5).all())  # every value is an exact tie
        return (torch.sign(v) * torch.floor(v.abs() + 0.5)).clamp(0, 255)

    mut = R.psnr_ref(away(o), away(t))
    assert (mut - ref).abs().item() > R.PSNR_TOL_DB
    assert (mut - ref).abs().item() > 1.0  # 3 dB in fact


def test_screened_inputs_are_off_ties():
    for ds in ("acdc", "dsb15"):
        o, t, mean, std = R.psnr_stats_case(ds)
        for x in (o, t):
            v = x.double() * R.f32(std) + R.f32(mean)
            assert bool((((v - torch.floor(v)) - 0.5).abs() >= 1e-3).all())
            # and so fp32 arithmetic, fused or not, rounds to the same grey level as fp64
            assert torch.equal((x * std + mean).round().clamp(0, 255).double(), R.denorm64(x, mean, std))
            fused = torch.addcmul(torch.tensor(R.f32(mean), dtype=torch.float64), x.double(),
                                  torch.tensor(R.f32(std), dtype=torch.float64)).float()
            assert torch.equal(fused.round().clamp(0, 255).double(), R.denorm64(x, mean, std))
