"""VAR.evidence_maps on CPU: evidence_maps_torch (the twin the kernels are held to bit for bit) against the reference's recorded
create_heatmaps_for_classes run (tests/golden/evidence_ref.npz, tools/gen_golden_evidence.py), its closed-form cases, the argument checks,
the colour table against matplotlib and the ABI of the new entry points."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT
from var_amd.models.var import EvidenceMaps, evidence_maps, evidence_maps_torch, jet_table

PNS10 = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
PNS5 = (1, 2, 3, 4, 5)


def L_of(pns):
    return sum(p * p for p in pns)


def synth_scores(N, K, pns, seed=0):
    """seeded scores shaped like log-probabilities: uniform in [-12, 0)"""
    return torch.from_numpy((-12.0 * np.random.default_rng(seed).random((N, K, L_of(pns)))).astype(np.float32))


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, 'evidence_ref.npz'))
    meta = json.loads(str(z['meta']))
    image = torch.from_numpy(z['image_k'].astype(np.float32) / np.float32(255))
    return z, meta, torch.from_numpy(z['scores']), image


def bins_of(v):
    return np.minimum((np.asarray(v, np.float32) * np.float32(256)).astype(np.int64), 255)


def check_against_fixture(r: EvidenceMaps, z, meta):
    """the three conditions of the fixture comparison, shared with the GPU test; returns the share of pixels whose bin differs"""
    K, size = meta['K'], meta['size']
    assert r.maps.shape == (1, K, size, size) and r.overlays.shape == (1, K, size, size, 3) and r.overlays.dtype == torch.uint8
    v = r.normalized()[0].cpu().numpy()
    d = np.abs(bins_of(v) - bins_of(z['norm']))
    share = float((d > 0).mean())
    assert d.max() <= 1, f'a colour bin differs by {d.max()}'
    assert share <= 0.01, f'{share:.4%} of the pixels fall in another bin'
    same = d == 0
    assert np.array_equal(r.overlays[0].cpu().numpy()[same], z['overlays'][same]), 'overlay bytes differ where the bins agree'
    # Two fp32 evaluations of the same map differ by at most the roundings of each.  A map value takes, per scale, 4 tap products, 2 + 1
    # row sums, 2 column products, the weight product and the accumulation: 11 roundings, 55 for the five selected scales, each on a
    # magnitude of at most max|score| (the weights l0 + l1 = 1 and sum w_s = 1 keep every intermediate inside the scores' range), so each
    # evaluation is within 55 * 2^-24 * max|score| of the exact value and two of them within 110 * 2^-24 * max|score| of each other.  lo and hi
    # are map values themselves: the same again for the numerator's m - lo, and the quotient by (hi - lo) and its rounding stay inside the
    # factor of 256 >= 2 * 110 + slack that the bar allows:  |v - norm| <= 256 * 2^-24 * max|score| / (hi - lo).
    sel = z['scores'][:, :sum(p * p for p in meta['patch_nums'][:len(meta['scales'])])]
    bound = 256 * 2.0 ** -24 * float(np.abs(sel).max()) / float(r.hi[0] - r.lo[0])
    err = float(np.abs(v.astype(np.float64) - z['norm'].astype(np.float64)).max())
    print(f'fixture: bins differ at {share:.4%} of the pixels, max |v - norm| = {err:.3e} (bound {bound:.3e})')
    assert err <= bound, f'|v - norm| = {err:.3e} exceeds {bound:.3e}'
    return share


def test_twin_against_the_reference_fixture(golden_dir):
    """The twin against the reference's own run: bins within 1 everywhere, different at no more than 1 % of the pixels, overlay bytes identical
    where the bins agree, and the normalised maps within 256 * 2^-24 * max|score| / (hi - lo) of the recorded ones.
    Measured on the CPU (torch 2.x, seed 7 of the generator): 0 of 131072 pixels in another bin (0.0000 %), all overlay bytes equal,
    max |v - norm| = 2.68e-07 against a bound of 2.52e-05; 17 % of the normalised values differ in their last bits."""
    z, meta, scores, image = load_fixture(golden_dir)
    assert tuple(meta['patch_nums']) == PNS10 and meta['image_range'] == '01'
    r = evidence_maps(scores, meta['patch_nums'], image=image, image_range='01', alpha=meta['alpha'], return_maps=True)
    assert r.scales == tuple(meta['scales']) == (0, 1, 2, 3, 4)
    check_against_fixture(r, z, meta)


def test_default_scales_are_the_first_half():
    for pns in (PNS5, PNS10, (1, 2, 3)):
        s = synth_scores(1, 2, pns)
        r = evidence_maps(s, pns, size=7, return_maps=True)
        assert r.scales == tuple(range(len(pns) // 2))
        assert torch.equal(r.maps, evidence_maps(s, pns, size=7, scales=range(len(pns) // 2), return_maps=True).maps)
    assert evidence_maps(s[0], (1, 2, 3), size=7).area.shape == (1, 2), 'a (K, L) input is one image'


def test_scale_0_alone_is_a_constant_map():
    """pn = 1: both taps are the one token, so the map is the score.  The axis table of the contract still carries l1 = src - i0 > 0 in the
    lower / right half (src = (d + 0.5) / size - 0.5 > 0 there, as in ATen), so the value is l0 * a + l1 * a with l0 = 1 - l1: four roundings
    (l0, two products, one sum), within 4 * 2^-24 |a| of a; where src clamps to 0 (l1 == 0: the upper / left half) it is a itself, bit for bit."""
    s = synth_scores(2, 3, PNS5)
    r = evidence_maps(s, PNS5, scales=(0,), size=20, return_maps=True)
    want = s[:, :, 0].reshape(2, 3, 1, 1).expand(2, 3, 20, 20)
    assert torch.equal(r.maps[:, :, :10, :10], want[:, :, :10, :10])
    assert bool(((r.maps - want).abs() <= 4 * 2.0 ** -24 * want.abs()).all())
    a = s[:, :, 0]
    assert bool(((r.lo - a.amin(1)).abs() <= 4 * 2.0 ** -24 * a.amin(1).abs()).all()) and bool(((r.hi - a.amax(1)).abs() <= 4 * 2.0 ** -24 * a.amax(1).abs()).all())
    assert torch.equal(r.pred, a.argmax(1).to(torch.int32).view(2, 1, 1).expand(2, 20, 20))


@pytest.mark.parametrize('si', [1, 2, 4])
def test_size_equal_to_pn_returns_the_scores(si):
    s = synth_scores(2, 3, PNS5, seed=si)
    pn = PNS5[si]
    b = L_of(PNS5[:si])
    r = evidence_maps(s, PNS5, scales=(si,), size=pn, return_maps=True)
    assert torch.equal(r.maps, s[:, :, b:b + pn * pn].view(2, 3, pn, pn))


@pytest.mark.parametrize('value,scales,size', [(0.0, None, 9), (-3.25, (2,), 3), (-3.25, (0,), 1)])
def test_flat_maps_take_table_entry_0(value, scales, size):
    """hi == lo: v = m - lo = 0, the table's entry 0 everywhere (maps that are flat bit for bit: zeros, or one scale at its own size)"""
    s = torch.full((1, 2, L_of(PNS5)), value)
    img = torch.zeros(3, size, size)
    r = evidence_maps(s, PNS5, scales=scales, size=size, image=img, image_range='01', alpha=1.0, return_maps=True)
    assert float(r.lo) == float(r.hi) == value
    assert torch.equal(r.normalized(), torch.zeros(1, 2, size, size))
    assert torch.equal(r.overlays, jet_table()[0].view(1, 1, 1, 1, 3).expand(1, 2, size, size, 3))
    assert torch.equal(r.pred, torch.zeros(1, size, size, dtype=torch.int32)) and torch.equal(r.margin, torch.zeros(1, size, size))


def test_one_class():
    s = synth_scores(2, 1, PNS5)
    r = evidence_maps(s, PNS5, size=20)
    assert torch.equal(r.margin, torch.full((2, 20, 20), math.inf)) and r.area.tolist() == [[400], [400]]
    assert torch.equal(r.pred, torch.zeros(2, 20, 20, dtype=torch.int32)) and r.maps is None and r.overlays is None
    with pytest.raises(ValueError):
        r.normalized()


def test_planted_tie_goes_to_the_lower_index():
    s = synth_scores(1, 4, PNS5)
    s[0, 3] = s[0, 1]                                    # classes 1 and 3 tie everywhere, exactly
    s[0, 1] += 20.0                                      # ... and win everywhere
    s[0, 3] = s[0, 1]
    r = evidence_maps(s, PNS5, size=20, scales=(0, 1, 2, 3, 4))
    assert torch.equal(r.pred, torch.ones(1, 20, 20, dtype=torch.int32)) and torch.equal(r.margin, torch.zeros(1, 20, 20))
    assert r.area.tolist() == [[0, 400, 0, 0]]


@pytest.mark.parametrize('pns,scales,size,N,K', [(PNS5, None, 37, 2, 5), (PNS10, tuple(range(10)), 20, 1, 7), (PNS5, (2, 4), 3, 3, 2)])
def test_pred_margin_and_area_follow_the_maps(pns, scales, size, N, K):
    s = synth_scores(N, K, pns, seed=3)
    r = evidence_maps(s, pns, scales=scales, size=size, return_maps=True)
    assert r.pred.dtype == torch.int32 and r.area.dtype == torch.int32 and r.margin.dtype == torch.float32
    assert torch.equal(r.area.sum(-1), torch.full((N,), size * size, dtype=torch.int64).to(r.area.sum(-1).dtype))
    top = torch.topk(r.maps, 2, dim=1).values
    assert torch.equal(r.margin, top[:, 0] - top[:, 1])
    assert torch.equal(r.maps.gather(1, r.pred.long().unsqueeze(1)).squeeze(1), top[:, 0])
    assert torch.equal(r.pred.long(), r.maps.argmax(1)) or bool((top[:, 0] == top[:, 1]).any())
    for n in range(N):
        assert torch.equal(r.area[n].long(), torch.bincount(r.pred[n].reshape(-1).long(), minlength=K))
    assert torch.equal(r.lo, r.maps.amin((1, 2, 3))) and torch.equal(r.hi, r.maps.amax((1, 2, 3)))
    nv = r.normalized()
    assert float(nv.min()) == 0.0 and float(nv.max()) == 1.0


def test_matches_interpolate():
    """the axis tables are torch's: F.interpolate(bilinear, align_corners=False), up and down, within fp32 rounding of the five-term sum"""
    s = synth_scores(1, 2, PNS10, seed=5)
    for size in (3, 20, 37, 256):
        r = evidence_maps(s, PNS10, scales=tuple(range(10)), size=size, return_maps=True)
        want = torch.zeros(1, 2, size, size, dtype=torch.float64)
        b = 0
        for p in PNS10:
            up = torch.nn.functional.interpolate(s[:, :, b:b + p * p].view(1, 2, p, p).double(), size=(size, size), mode='bilinear', align_corners=False)
            want += up * (p * p / L_of(PNS10))
            b += p * p
        assert float((r.maps.double() - want).abs().max()) <= 110 * 2.0 ** -24 * 12.0 * 2


def test_overlay_steps_in_numpy():
    """the overlay, step by step as the issue of this feature states it, in numpy on the twin's maps; both image ranges, four alphas"""
    s = synth_scores(2, 3, PNS5, seed=9)
    rng = np.random.default_rng(1)
    jet = jet_table().numpy()
    for image_range, alpha in (('01', 0.5), ('pm1', 0.3), ('pm1', 0.0), ('01', 1.0)):
        img = rng.random((2, 3, 20, 20)).astype(np.float32)
        if image_range == 'pm1':
            img = img * np.float32(2) - np.float32(1)
        r = evidence_maps(s, PNS5, size=20, image=torch.from_numpy(img), image_range=image_range, alpha=alpha, return_maps=True)
        for n in range(2):
            m = r.maps[n].numpy()
            lo, hi = m.min(), m.max()
            v = (m - lo) / (hi - lo)
            col = jet[bins_of(v)]
            x = (img[n] + np.float32(1)) / np.float32(2) if image_range == 'pm1' else img[n]
            i8 = (x.transpose(1, 2, 0) * np.float32(255)).astype(np.uint8)
            want = np.clip(i8 * (1 - alpha) + col * alpha, 0, 255).astype(np.uint8)
            assert np.array_equal(r.overlays[n].numpy(), want), (image_range, alpha, n)


def test_argument_checks():
    s = synth_scores(2, 3, PNS5)
    img = torch.zeros(2, 3, 8, 8)
    ok = dict(size=8)
    evidence_maps(s, PNS5, image=img, **ok)
    bad_scores = (s[..., :-1], s.double(), s[0, 0], s.view(1, 2, 3, -1), s.numpy(), s[:0])
    for b in bad_scores:
        with pytest.raises(ValueError):
            evidence_maps(b, PNS5, **ok)
    for sc in ((), (5,), (-1,), (1, 1), (2, 1), (0, 1.5), 'ab', 3, (True,)):
        with pytest.raises(ValueError):
            evidence_maps(s, PNS5, scales=sc, **ok)
    with pytest.raises(ValueError):
        evidence_maps(torch.zeros(1, 1, 1), (1,))                        # one scale: the default selection is empty
    for size in (0, -3, 2.5, True, 4097):
        with pytest.raises(ValueError):
            evidence_maps(s, PNS5, size=size)
    for a in (-0.01, 1.01, math.nan, math.inf, '0.5', None, True):
        with pytest.raises(ValueError):
            evidence_maps(s, PNS5, image=img, alpha=a, **ok)
    with pytest.raises(ValueError):
        evidence_maps(s, PNS5, image=img, image_range='0255', **ok)
    for im in (img[:1], img[0], torch.zeros(2, 3, 8, 9), torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.uint8), img.numpy()):
        with pytest.raises(ValueError):
            evidence_maps(s, PNS5, image=im, **ok)
    evidence_maps(s[0], PNS5, image=img[0], **ok)                        # (K, L) with (3, size, size) is one image
    for v in (math.nan, math.inf, -math.inf):
        t = s.clone()
        t[1, 2, 3] = v
        with pytest.raises(ValueError):
            evidence_maps(t, PNS5, **ok)
        evidence_maps(t, PNS5, check=False, **ok)                        # skipped on request (the result is undefined)
        evidence_maps(t, PNS5, scales=(3,), **ok)                        # only the selected scales are tested


def test_model_methods(golden_dir):
    """VAR.evidence_maps passes the model's patch_nums; VAR.class_heatmaps is token_scores followed by evidence_maps"""
    from tests.test_token_scores_cpu import fixture_model
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    pns = tuple(var.patch_nums)
    lp = var.token_log_likelihood(gt, [3, 5])
    img = torch.rand(gt.shape[0], 3, 12, 12, generator=torch.Generator().manual_seed(0)) * 2 - 1
    a = var.class_heatmaps(gt, [3, 5], img, size=12, return_maps=True, alpha=0.3)
    b = evidence_maps(lp, pns, size=12, image=img, return_maps=True, alpha=0.3)
    for f in ('lo', 'hi', 'pred', 'margin', 'area', 'maps', 'overlays'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.patch_nums == pns and a.size == 12 and 'EvidenceMaps(images=' in repr(a)
    c = var.class_heatmaps(gt, [3, 5], img, score='group_smoothed', group=7, size=12, scales=(1, 2), image_range='pm1')
    d = var.evidence_maps(var.token_scores(gt, [3, 5], 'group_smoothed', group=7), size=12, scales=(1, 2), image=img)
    assert torch.equal(c.overlays, d.overlays) and torch.equal(c.pred, d.pred)
    import models.var
    assert models.var.EvidenceMaps is EvidenceMaps and models.var.evidence_maps_torch is evidence_maps_torch


def test_jet_table_is_matplotlibs():
    matplotlib = pytest.importorskip('matplotlib')
    want = (matplotlib.colormaps['jet'](np.arange(256))[:, :3] * 255).astype(np.uint8)
    got = jet_table().numpy()
    assert got.shape == (256, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    # ... and the float path the fork takes, (cmap(v)[..., :3] * 255).astype(uint8), picks entry min(int(v * 256), 255)
    v = np.concatenate([np.linspace(0, 1, 1001, dtype=np.float32), np.float32([1.0, 0.999999, 0.00390625])])
    assert np.array_equal((matplotlib.colormaps['jet'](v)[..., :3] * 255).astype(np.uint8), got[bins_of(v)])


def test_abi_of_the_new_entry_points():
    from var_amd import abi, hip
    for name in ('evidence_reduce_f32', 'evidence_overlay_u8'):       # (the argument lists: tests/test_abi_cpu.py, for every declaration)
        assert name in abi.SIGNATURES_HIP_ONLY and name in hip.lib().fn
    assert 'evidence_jet_host' in abi.SIGNATURES_HOST and 'evidence_jet_host' in hip.lib().host
    # the launchers refuse what the header says they refuse, before anything touches a GPU
    z = ctypes.c_void_p(0)
    one = (ctypes.c_int * 1)(1)
    assert hip.lib().fn['evidence_reduce_f32'](z, 1, 1, 1, 1, 1, one, one, one, z, z, 4, z, z, z, z, z, z, z) == abi.EINVAL
    assert hip.lib().fn['evidence_overlay_u8'](z, 1, 1, 1, 1, 1, one, one, one, z, z, 4, z, z, z, 0, 0.5, z, z) == abi.EINVAL
