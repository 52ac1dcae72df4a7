"""Per-image sampling on the GPU: the Philox Exp(1) fill against its host twin, the per-image sampler entry against the scalar
one image by image, and VAR.autoregressive_infer_cfg_per_image — batch invariance in the three precisions, the CPU oracle at B = 1, the
existing engine path on the same noise, and no side effects on the plain call."""
import contextlib
import io

import numpy as np
import pytest

from tests import util
from tests.test_per_image_cpu import host_fill

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PNS, DEPTH, CH = (1, 2, 3, 4), 2, 32
_MODELS = {}


def _hip():
    from var_amd import hip
    return hip


def _model():
    if 'm' not in _MODELS:
        from models import build_vae_var
        from var_amd.detinit import fill_module_device_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=DEPTH, ch=CH)
        fill_module_device_(var, DEPTH, 0, 'var.'); fill_module_device_(vae, DEPTH, 0, 'vae.')
        _MODELS['m'] = (vae.eval(), var.eval())
    return _MODELS['m']


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- (a) the fill -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B, l, V', [(3, 1, 4096), (5, 169, 4096), (2, 16, 8192), (4, 9, 256)])
def test_device_fill_equals_the_host_twin(B, l, V):
    seeds = [(0x9E3779B97F4A7C15 * (b + 1)) % (1 << 63) for b in range(B)]
    seeds[0] = 0
    sd = torch.tensor(seeds, dtype=torch.int64, device='cuda')
    for scale, draw in [(0, 0), (0, 1), (3, 0), (9, 1), (31, 0)]:
        out = torch.full((B * l, V), float('nan'), device='cuda')
        util.guarded_call('exp1_philox_f32', sd, B, l, V, scale, draw, out)
        want = host_fill(seeds, l, V, scale, draw)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), (scale, draw)


def test_fill_rejects_bad_arguments():
    hip = _hip()
    sd = torch.zeros(2, dtype=torch.int64, device='cuda')
    out = torch.zeros(64, device='cuda')
    for args in [(sd, 0, 1, 4, 0, 0, out), (sd, 1, 0, 4, 0, 0, out), (sd, 1, 1, 6, 0, 0, out), (sd, 1, 1, 4, -1, 0, out), (sd, 1, 1, 4, 0, 0, out[1:])]:
        with pytest.raises(hip.VarHipError, match='EINVAL'):
            hip.call('exp1_philox_f32', *args)


# ---- (b) the per-image sampler entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [4096, 1024])
def test_rows_entry_equals_the_scalar_entry_image_by_image(V):
    """every (top_k, top_p, t) combination as one image of a single launch; row 0 of an image is a random row, row 1 takes three distinct values
    (more than a thousand exact ties with the k-th value: under the scalar entry's own sort buffer of 1024 entries the tie crowd is walked
    unsorted, under this launch's buffer of V entries it is sorted — the results must not differ), row 2 is constant"""
    hip = _hip()
    combos = [(k, p, t) for k in (0, 1, 900, V) for p in (0.0, 0.96, 1.0) for t in (0.0, 0.75, 4.0)]
    B, l = len(combos), 3
    g = torch.Generator().manual_seed(V)
    logits = torch.randn(2, B, l, V, generator=g) * 3
    logits[:, :, 1] = torch.randint(0, 3, (2, B, V), generator=g).float()
    logits[:, :, 2] = 0.25
    logits = logits.view(2 * B * l, V).cuda()
    noise = torch.empty(B * l, V).exponential_(1, generator=g).cuda()
    tk = torch.tensor([c[0] for c in combos], dtype=torch.int32, device='cuda')
    tp = torch.tensor([c[1] for c in combos], dtype=torch.float64, device='cuda')
    tt = torch.tensor([c[2] for c in combos], dtype=torch.float64, device='cuda')
    narrow = [b for b, c in enumerate(combos) if c[0] in (1, 900)]           # a launch whose sort buffer is the scalar entry's (cap 1024)
    try:
        for walk in (0, 1):
            hip.lib().so.varhip_sampler_force_walk(walk)
            idx = torch.full((B * l,), -7, dtype=torch.int64, device='cuda')
            masked = torch.full((B * l, V), float('nan'), device='cuda')
            util.guarded_call('cfg_sample_rows_f32', logits, noise, idx, masked, B, l, V, tt, tk, tp, V)
            assert int(idx.min()) >= 0 and int(idx.max()) < V
            lg4 = logits.view(2, B, l, V)
            for b, (k, p, t) in enumerate(combos):
                one = lg4[:, b].contiguous().view(2 * l, V)
                i1 = torch.full((l,), -7, dtype=torch.int64, device='cuda')
                m1 = torch.full((l, V), float('nan'), device='cuda')
                util.guarded_call('cfg_sample_f32', one, noise[b * l:(b + 1) * l].contiguous(), i1, m1, 1, l, V, t, k, p)
                assert torch.equal(i1, idx[b * l:(b + 1) * l]), (walk, b, combos[b], i1, idx[b * l:(b + 1) * l])
                assert torch.equal(_bits(m1), _bits(masked[b * l:(b + 1) * l])), (walk, b, combos[b])
            sel = torch.tensor(narrow, device='cuda')
            lg_n = lg4[:, sel].contiguous().view(-1, V)
            i2 = torch.full((len(narrow) * l,), -7, dtype=torch.int64, device='cuda')
            m2 = torch.full((len(narrow) * l, V), float('nan'), device='cuda')
            util.guarded_call('cfg_sample_rows_f32', lg_n, noise.view(B, l, V)[sel].contiguous().view(-1, V), i2, m2, len(narrow), l, V,
                              tt[sel].contiguous(), tk[sel].contiguous(), tp[sel].contiguous(), 900)
            assert torch.equal(i2.view(-1, l), idx.view(B, l)[sel]) and torch.equal(_bits(m2).view(len(narrow), l, V), _bits(masked).view(B, l, V)[sel])
    finally:
        hip.lib().so.varhip_sampler_force_walk(0)


def test_rows_entry_refuses_what_does_not_fit():
    hip = _hip()
    V, B, l = 1024, 2, 1
    logits = torch.randn(2 * B * l, V, device='cuda')
    noise = torch.empty(B * l, V, device='cuda').exponential_(1)
    idx = torch.zeros(B * l, dtype=torch.int64, device='cuda')
    z = torch.zeros(B, dtype=torch.float64, device='cuda')
    k = torch.tensor([5, 900], dtype=torch.int32, device='cuda')
    for cap in (0, V + 1):
        with pytest.raises(hip.VarHipError, match='EINVAL'):
            hip.call('cfg_sample_rows_f32', logits, noise, idx, None, B, l, V, z, k, z, cap)
    util.guarded_call('cfg_sample_rows_f32', logits, noise, idx, None, B, l, V, z, k, z, 8)       # image 1 needs more than the launch was sized for
    assert int(idx[0]) >= 0 and int(idx[1]) == -1


# ---- (c) - (f) the public call ------------------------------------------------------------------------------------------------------------
DECK = dict(labels=[3, 980, 22, 1000, 417, 207], seeds=[17, 3, (1 << 62) + 5, 0, 99991, 17],
            cfg=[4.0, 1.5, 0.0, 2.5, 1.5, 3.0], top_k=[0, 900, 1, 900, 0, 600], top_p=[0.96, 0.0, 0.0, 0.96, 0.0, 0.5])
N = len(DECK['labels'])


def _call(var, ids, more_smooth=False):
    d = DECK
    img, tok = var.autoregressive_infer_cfg_per_image(torch.tensor([d['labels'][i] for i in ids]), [d['seeds'][i] for i in ids],
                                                      cfg=[d['cfg'][i] for i in ids], top_k=[d['top_k'][i] for i in ids],
                                                      top_p=[d['top_p'][i] for i in ids], more_smooth=more_smooth, return_tokens=True)
    return img.clone(), tok.clone()


PIXEL_BOUND = {'f32': 2e-5, 'f16': 5e-3, 'bf16': 4e-2}


@pytest.mark.parametrize('prec, more_smooth', [('f32', False), ('f16', False), ('bf16', False), ('f32', True), ('f16', True)])
def test_requests_do_not_depend_on_their_batch(prec, more_smooth):
    """six requests: in one batch, in one batch in another order, split 1 + 2 + 3, and each alone.  Tokens: bit-equal.  Pixels: f32 within twice
    the 1e-5 each grouping owes the oracle; 16-bit within the bounds of the sub-batch checks of tests/test_f16_gpu.py (the decoder's kernel
    choice follows the batch)"""
    vae, var = _model()
    var.set_hip_precision(prec)
    try:
        img, tok = _call(var, list(range(N)), more_smooth)
        assert img.shape == (N, 3, 64, 64) and tok.shape == (N, 30) and torch.isfinite(img).all()
        perm = [4, 0, 2, 5, 1, 3]
        groupings = {'permuted': [perm], 'split 1+2+3': [[0], [1, 2], [3, 4, 5]], 'alone': [[i] for i in range(N)]}
        worst = 0.0
        for name, groups in groupings.items():
            for ids in groups:
                gi, gt = _call(var, ids, more_smooth)
                for j, i in enumerate(ids):
                    assert torch.equal(gt[j], tok[i]), f'{prec} {name}: tokens of request {i} changed with its batch'
                    worst = max(worst, float((gi[j] - img[i]).abs().max()))
        print(f'{prec} more_smooth={more_smooth}: max pixel difference across groupings {worst:.3e}')
        assert worst <= PIXEL_BOUND[prec], worst
        assert len({tuple(t.tolist()) for t in tok}) == N
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('more_smooth', [False, True])
def test_requests_equal_the_oracle_at_batch_one(more_smooth):
    from tests.test_per_image_cpu import _oracle, oracle_request
    vae, var = _model()
    img, tok = _call(var, list(range(N)), more_smooth)
    orc = _oracle()
    d = DECK
    for b in range(N):
        ref = oracle_request(orc, d['labels'][b], d['seeds'][b], d['cfg'][b], d['top_k'][b], d['top_p'][b], more_smooth)
        assert np.array_equal(tok[b].cpu().numpy(), ref['idx'][0]), (b, tok[b], ref['idx'][0])
        ok, msg = util.diff_report(f'request {b}', img[b].cpu().numpy(), ref['img'][0], atol=1e-5)
        assert ok, msg


def test_requests_equal_the_scalar_engine_path_on_their_noise():
    vae, var = _model()
    eng = var.engine()
    _, tok = _call(var, list(range(N)))
    d = DECK
    for b in range(N):
        noise = [torch.from_numpy(host_fill([d['seeds'][b]], pn * pn, var.V, si, 0)) for si, pn in enumerate(PNS)]
        eng.sample(1, torch.tensor([d['labels'][b]], device='cuda'), None, d['cfg'][b], d['top_k'][b], d['top_p'][b], noises=noise, trace=True)
        assert torch.equal(torch.cat(eng.last_trace['idx'], dim=1)[0], tok[b]), b


def test_no_side_effects_between_the_plain_and_the_per_image_call():
    vae, var = _model()
    labels = torch.tensor([3, 7, 980], device='cuda')
    plain = lambda: var.autoregressive_infer_cfg(3, labels, g_seed=0, cfg=1.5, top_k=900, top_p=0.96).clone()
    a = plain()
    state = var.rng.get_state().clone()
    p1 = _call(var, [0, 1, 2, 3])
    assert torch.equal(var.rng.get_state(), state), 'the per-image call must not touch the model generator'
    b = plain()
    p2 = _call(var, [0, 1, 2, 3])
    assert torch.equal(a, b), 'the plain call changed after a per-image call'
    assert torch.equal(p1[0], p2[0]) and torch.equal(p1[1], p2[1]), 'the per-image call changed after a plain call'
    ms = lambda: var.autoregressive_infer_cfg(3, labels, g_seed=0, cfg=1.5, top_k=900, top_p=0.96, more_smooth=True).clone()
    c = ms(); _call(var, [4, 5], more_smooth=True); assert torch.equal(c, ms())


def test_uniform_parameters_and_validation_on_the_device():
    vae, var = _model()
    a = var.autoregressive_infer_cfg_per_image([5, 6, 7], [1, 2, 3], cfg=2.0, top_k=900, top_p=0.96, return_tokens=True)
    b = var.autoregressive_infer_cfg_per_image(torch.tensor([5, 6, 7], device='cuda'), torch.tensor([1, 2, 3]), cfg=[2.0] * 3, top_k=[900] * 3,
                                               top_p=[0.96] * 3, return_tokens=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in [dict(g_seeds=[0, 1]), dict(top_k=[0, 1, var.V + 1]), dict(top_p=1.5), dict(cfg=float('nan')), dict(g_seeds=[0, 1, -2]), dict(label_B=[1, 2, 1001])]:
        with pytest.raises(ValueError):
            var.autoregressive_infer_cfg_per_image(**{**dict(label_B=[5, 6, 7], g_seeds=[1, 2, 3]), **bad})
