"""VAR.evidence_maps on the MI355X: varhip_evidence_reduce_f32 and varhip_evidence_overlay_u8 against evidence_maps_torch on the CPU, every
field bit for bit and the overlays byte for byte, on every path of the kernels (the three scale / stage buckets, pixel tiles that end inside
a workgroup, size < pn, the packed store's unaligned head and tail, the LDS and the global area histogram, the class loop's double buffer
over odd and even counts), batch and history independence, the workgroup min / max, the reference's fixture and the model-level call.

Kernel-level calls go through util.guarded_call with every output prefilled (NaN / 0xFF): a cell the kernels leave out fails its comparison,
a store outside an operand fails the band check."""
import contextlib
import io
import itertools
import json

import numpy as np
import pytest
import torch

from tests import util
from tests.test_evidence_cpu import PNS5, PNS10, L_of, check_against_fixture, load_fixture, synth_scores
from var_amd import abi, engine, hip
from var_amd.models.var import evidence_maps, evidence_maps_torch

pytestmark = pytest.mark.gpu

FIELDS = ('lo', 'hi', 'pred', 'margin', 'area', 'maps', 'overlays')
ALPHAS = (0.0, 0.5, 0.3, 1.0)


def synth_image(N, size, pm1, seed):
    x = np.random.default_rng(seed).random((N, 3, size, size)).astype(np.float32)
    return torch.from_numpy(x * np.float32(2) - np.float32(1) if pm1 else x)


def run_kernels(scores, pns, scales, size, image=None, pm1=True, alpha=0.5, return_maps=False):
    """the two entry points, guarded, on prefilled outputs -> dict of CPU tensors (the fields of evidence_maps_torch)"""
    N, K, L = scores.shape
    sd = scores.cuda()
    pn, begin, w = engine.evidence_scales(pns, scales)
    ax_i, ax_l = engine.evidence_axis_tables(tuple(pn.tolist()), size, sd.device)
    host = (torch.from_numpy(pn), torch.from_numpy(begin), torch.from_numpy(w))
    nan = float('nan')
    out = dict(lo=torch.full((N,), nan, device='cuda'), hi=torch.full((N,), nan, device='cuda'),
               pred=torch.full((N, size, size), -1, dtype=torch.int32, device='cuda'), margin=torch.full((N, size, size), nan, device='cuda'),
               area=torch.full((N, K), -1, dtype=torch.int32, device='cuda'),
               maps=torch.full((N, K, size, size), nan, device='cuda') if return_maps else None, overlays=None)
    util.guarded_call('evidence_reduce_f32', sd, K * L, L, N, K, len(pn), *host, ax_i, ax_l, size,
                      out['lo'], out['hi'], out['pred'], out['margin'], out['area'], out['maps'])
    if image is not None:
        # 0xFF prefill, and 0x5A under it once more: a byte the kernel leaves out cannot pass as a white pixel in both runs
        for fill in (0xFF, 0x5A):
            out['overlays'] = torch.full((N, K, size, size, 3), fill, dtype=torch.uint8, device='cuda')
            util.guarded_call('evidence_overlay_u8', sd, K * L, L, N, K, len(pn), *host, ax_i, ax_l, size,
                              out['lo'], out['hi'], image.cuda(), 1 if pm1 else 0, float(alpha), out['overlays'])
            out[f'overlays_{fill}'] = out['overlays'].cpu()
        assert torch.equal(out.pop('overlays_255'), out.pop('overlays_90')), 'the overlay depends on what the output held'
    torch.cuda.synchronize()
    return {k: (v.cpu() if v is not None else None) for k, v in out.items()}


def assert_same(got, want, what=''):
    for f in FIELDS:
        g, w = got[f], want[f]
        assert (g is None) == (w is None), (what, f)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype, g.shape, w.shape)
            if g.dtype.is_floating_point:
                g, w = g.view(torch.int32), w.view(torch.int32)                 # bit for bit
            nbad = int((g != w).sum())
            assert nbad == 0, f'{what}: {f} differs at {nbad} of {g.numel()} elements'


def scale_sets(pns):
    S = len(pns)
    return {'first': (0,), 'two': (2, 4), 'default': tuple(range(S // 2)), 'all': tuple(range(S))}


CASES = list(itertools.product((PNS5, PNS10), (3, 20, 37, 256), (1, 2, 37), ('first', 'two', 'default', 'all')))


@pytest.mark.parametrize('ci', range(len(CASES)), ids=[f'pn{len(c[0])}-s{c[1]}-K{c[2]}-{c[3]}' for c in CASES])
def test_kernels_against_the_twin(ci):
    """patch_nums x size x K x scales in full; N, the image (none / pm1 / 01), alpha and return_maps cycle through the cases so that every
    value of each meets every size and every K"""
    pns, size, K, sname = CASES[ci]
    scales = scale_sets(pns)[sname]
    N = (1, 3)[(ci + ci // 4) % 2]
    mode = (ci + ci // 12) % 3                       # 0: no image, 1: pm1, 2: 01
    alpha = ALPHAS[(ci + ci // 3) % 4]
    return_maps = bool((ci + ci // 2) % 2)
    scores = synth_scores(N, K, pns, seed=ci)
    image = None if mode == 0 else synth_image(N, size, mode == 1, ci)
    want = evidence_maps_torch(scores, pns, scales, size, image, mode == 1, alpha, return_maps)
    got = run_kernels(scores, pns, scales, size, image, mode == 1, alpha, return_maps)
    assert_same(got, want, f'N={N} mode={mode} alpha={alpha} maps={return_maps}')
    assert int(got['area'].sum()) == N * size * size


@pytest.mark.parametrize('alpha', ALPHAS)
@pytest.mark.parametrize('pm1', [True, False])
def test_overlay_every_alpha_and_range(alpha, pm1):
    """an odd size with K = 3: the maps' first bytes sit at every alignment (1369 * 3 bytes per map), images with values beyond their range"""
    scores = synth_scores(2, 3, PNS5, seed=11)
    image = synth_image(2, 37, pm1, 5) * 1.25
    want = evidence_maps_torch(scores, PNS5, (0, 1), 37, image, pm1, alpha, True)
    assert_same(run_kernels(scores, PNS5, (0, 1), 37, image, pm1, alpha, True), want, f'alpha {alpha} pm1 {pm1}')


@pytest.mark.parametrize('size', [1, 2, 5])
def test_tiny_sizes(size):
    """fewer pixels than one packed group, with and without an aligned group in a map"""
    scores = synth_scores(3, 5, PNS5, seed=size)
    image = synth_image(3, size, False, size)
    want = evidence_maps_torch(scores, PNS5, (0, 1, 2), size, image, False, 0.5, True)
    assert_same(run_kernels(scores, PNS5, (0, 1, 2), size, image, False, 0.5, True), want, f'size {size}')


def test_more_classes_than_the_lds_histogram():
    """K = 4097 > 4096: the area goes through global atomics; an even K below it for the double buffer"""
    for K in (4097, 64):
        scores = synth_scores(1, K, PNS5, seed=K)
        want = evidence_maps_torch(scores, PNS5, (0, 1), 20, None, True, 0.5, False)
        got = run_kernels(scores, PNS5, (0, 1), 20)
        assert_same(got, want, f'K {K}')
        assert int(got['area'].sum()) == 400


def test_twelve_scales_take_the_widest_instantiation():
    """more than 10 selected scales (and 650 staged tokens): the <16, 16> kernels"""
    pns = tuple(range(1, 13))
    scores = synth_scores(2, 3, pns, seed=12)
    image = synth_image(2, 20, True, 12)
    want = evidence_maps_torch(scores, pns, tuple(range(12)), 20, image, True, 0.5, True)
    assert_same(run_kernels(scores, pns, tuple(range(12)), 20, image, True, 0.5, True), want)
    # ... and few scales spanning more than 768 tokens
    pns = (1, 20, 30)
    scores = synth_scores(1, 2, pns, seed=13)
    want = evidence_maps_torch(scores, pns, (0, 2), 37, None, True, 0.5, True)
    assert_same(run_kernels(scores, pns, (0, 2), 37, return_maps=True), want)


def test_extremes_in_the_last_partial_tile():
    """400 pixels = one full workgroup and one of 144: one scale at its own size, so the map is the scores; the maximum only at the last pixel,
    the minimum only at pixel 300, and in the second image both in the first workgroup: a lost workgroup min / max shows in lo / hi"""
    pns = (1, 20)
    scores = synth_scores(2, 2, pns, seed=3)
    scores[0, 1, 1 + 399] = 7.5
    scores[0, 0, 1 + 300] = -40.0
    scores[1, 0, 1 + 5] = 9.25
    scores[1, 1, 1 + 255] = -33.0
    got = run_kernels(scores, pns, (1,), 20, return_maps=True)
    assert got['lo'].tolist() == [-40.0, -33.0] and got['hi'].tolist() == [7.5, 9.25]
    assert torch.equal(got['maps'], scores[:, :, 1:].view(2, 2, 20, 20))
    assert_same(got, evidence_maps_torch(scores, pns, (1,), 20, None, True, 0.5, True))


def test_planted_tie_and_one_class():
    s = synth_scores(1, 4, PNS5)
    s[0, 1] += 20.0
    s[0, 3] = s[0, 1]
    got = run_kernels(s, PNS5, (0, 1, 2, 3, 4), 20)
    assert torch.equal(got['pred'], torch.ones(1, 20, 20, dtype=torch.int32)) and torch.equal(got['margin'], torch.zeros(1, 20, 20))
    assert got['area'].tolist() == [[0, 400, 0, 0]]
    one = run_kernels(s[:, :1], PNS5, (0, 1), 20)
    assert torch.equal(one['margin'], torch.full((1, 20, 20), float('inf'))) and one['area'].tolist() == [[400]]


def test_batch_and_history_independence():
    """image n of a batch equals the image alone; a repeated call is bit-equal; a call after another size, and another scale set at the same
    size, finds its own axis tables"""
    pns = PNS10
    scores = synth_scores(3, 5, pns, seed=21).cuda()
    image = synth_image(3, 37, True, 21).cuda()

    def fields(r):
        return {f: (getattr(r, f).cpu() if getattr(r, f) is not None else None) for f in FIELDS}
    a = fields(evidence_maps(scores, pns, size=37, image=image, return_maps=True))
    assert_same(a, evidence_maps_torch(scores.cpu(), pns, tuple(range(5)), 37, image.cpu(), True, 0.5, True), 'model-level call')
    assert_same(fields(evidence_maps(scores, pns, size=37, image=image, return_maps=True)), a, 'second call')
    for n in range(3):
        b = fields(evidence_maps(scores[n:n + 1], pns, size=37, image=image[n:n + 1], return_maps=True))
        assert_same(b, {f: a[f][n:n + 1] for f in FIELDS}, f'image {n} alone')
    other = fields(evidence_maps(scores, pns, size=20, return_maps=True))
    assert_same(other, evidence_maps_torch(scores.cpu(), pns, tuple(range(5)), 20, None, True, 0.5, True), 'after a call with another size')
    assert_same(fields(evidence_maps(scores, pns, size=37, image=image, return_maps=True)), a, 'back at the first size')
    sub = fields(evidence_maps(scores, pns, size=37, scales=(1, 3), return_maps=True))
    assert_same(sub, evidence_maps_torch(scores.cpu(), pns, (1, 3), 37, None, True, 0.5, True), 'other scales at the same size')
    with pytest.raises(ValueError):
        bad = scores.clone()
        bad[2, 4, 17] = float('nan')
        evidence_maps(bad, pns, size=37)
    evidence_maps(scores, pns, size=37, check=False)


def test_fixture_on_the_gpu(golden_dir):
    """the reference's recorded run, the three conditions of the CPU test, through the kernels"""
    z, meta, scores, image = load_fixture(golden_dir)
    r = evidence_maps(scores.cuda(), meta['patch_nums'], image=image.cuda(), image_range='01', alpha=meta['alpha'], return_maps=True)
    assert r.overlays.is_cuda and r.maps.is_cuda
    check_against_fixture(r, z, meta)
    want = evidence_maps_torch(scores.unsqueeze(0), meta['patch_nums'], tuple(meta['scales']), meta['size'], image.unsqueeze(0), False, meta['alpha'], True)
    assert_same({f: getattr(r, f).cpu() for f in FIELDS}, want, 'fixture inputs')


def test_launchers_refuse_bad_arguments():
    N, K, size = 2, 3, 8
    L = L_of(PNS5)
    sc = torch.zeros(N, K, L, device='cuda')
    pn, begin, w = engine.evidence_scales(PNS5, (1, 2))
    ax_i, ax_l = engine.evidence_axis_tables((2, 3), size, sc.device)
    lo, hi = torch.zeros(N, device='cuda'), torch.zeros(N, device='cuda')
    pred = torch.zeros(N, size, size, dtype=torch.int32, device='cuda'); margin = torch.zeros(N, size, size, device='cuda')
    area = torch.zeros(N, K, dtype=torch.int32, device='cuda')
    img = torch.zeros(N, 3, size, size, device='cuda'); out = torch.zeros(N, K, size, size, 3, dtype=torch.uint8, device='cuda')
    p = lambda a: a.ctypes.data                                                       # noqa: E731
    st = hip.current_stream()
    red = [sc.data_ptr(), K * L, L, N, K, 2, p(pn), p(begin), p(w), ax_i.data_ptr(), ax_l.data_ptr(), size,
           lo.data_ptr(), hi.data_ptr(), pred.data_ptr(), margin.data_ptr(), area.data_ptr(), None]
    ovl = red[:12] + [lo.data_ptr(), hi.data_ptr(), img.data_ptr(), 0, 0.5, out.data_ptr()]
    f, g = hip.lib().fn['evidence_reduce_f32'], hip.lib().fn['evidence_overlay_u8']
    assert f(*red, st) == 0 and g(*ovl, st) == 0
    torch.cuda.synchronize()
    over, neg = np.asarray([2, 3], np.int32), np.asarray([-1, 5], np.int32)
    big = np.asarray([2, 65], np.int32)
    nanw = np.asarray([0.5, np.nan], np.float32)
    common = [(0, None), (1, K * L - 1), (2, 13), (3, 0), (4, 0), (5, 0), (5, 17), (6, None), (6, p(big)), (7, p(over)), (7, p(neg)), (8, p(nanw)),
              (9, None), (10, None), (11, 0), (11, 4097), (12, None), (13, None)]
    for pos, val in common + [(3, 65536), (14, None), (15, None), (16, None)]:
        a = list(red); a[pos] = val
        assert f(*a, st) == abi.EINVAL, ('reduce', pos, val)
    for pos, val in common + [(14, None), (15, 2), (16, 1.5), (16, -0.1), (16, float('nan')), (17, None)]:
        a = list(ovl); a[pos] = val
        assert g(*a, st) == abi.EINVAL, ('overlay', pos, val)
    with pytest.raises(ValueError):
        evidence_maps(torch.zeros(1, 1, 1 + 70 * 70, device='cuda'), (1, 70), scales=(0, 1), size=8)     # a scale the kernels do not take


def test_class_heatmaps_end_to_end(golden_dir):
    """var.class_heatmaps on the d2 fixture model equals evidence_maps(token_log_likelihood(...)), on the HIP route of both"""
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    z = np.load(f'{golden_dir}/encode_t_pn12345.npz')
    meta = json.loads(str(z['meta']))
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
    fill_module_(var, meta['depth'], 0, 'var.'); fill_module_(vae, meta['depth'], 0, 'vae.')
    var.eval()
    gt = torch.from_numpy(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], 1).astype(np.int64)).cuda()
    image = synth_image(gt.shape[0], 40, True, 1).cuda()
    classes = [3, meta['labels'][0], 999]
    a = var.class_heatmaps(gt, classes, image, size=40, return_maps=True)
    lp = var.token_log_likelihood(gt, classes)
    assert lp.is_cuda and var._scoring_on_hip(gt)
    b = var.evidence_maps(lp, size=40, image=image, return_maps=True)
    got = {f: getattr(a, f).cpu() for f in FIELDS}
    assert_same(got, {f: getattr(b, f).cpu() for f in FIELDS}, 'class_heatmaps')
    assert_same(got, evidence_maps_torch(lp.cpu(), var.patch_nums, (0, 1), 40, image.cpu(), True, 0.5, True), 'against the twin')
    assert a.overlays.shape == (gt.shape[0], 3, 40, 40, 3) and int(a.area.sum()) == gt.shape[0] * 1600
