"""VAR.abduct_noise / VAR.counterfactual on the MI355X, d2 test model.  The tokens come from a per-image sampling call, so their
source distribution is the model's own: replayed under the same label the abducted noise must give them back bit for bit."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PNS, DEPTH, CH = (1, 2, 3, 4, 5), 2, 32
S = len(PNS)
_MODELS, _SRC = {}, {}
LABELS, SEEDS, CFG = [3, 980, 22, 1000, 7, 512], [17, 3, (1 << 62) + 5, 0, 99, 12345], [4.0, 1.5, 0.0, 2.5, 1.5, 3.0]
DST = [980, 3, 7, 22, 1000, 3]
ABD_SEEDS = [5, 6, 7, (1 << 61) + 1, 9, 10]
# the precisions' pixel bounds of the per-image call's batch invariance (tests/test_per_image_gpu.py: PIXEL_BOUND)
PIXEL = {'f32': 2e-5, 'bf16': 4e-2}


def _model(seed=0):
    if seed not in _MODELS:
        from models import build_vae_var
        from var_amd.detinit import fill_module_device_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=DEPTH, ch=CH)
        fill_module_device_(var, DEPTH, seed, 'var.'); fill_module_device_(vae, DEPTH, seed, 'vae.')
        _MODELS[seed] = (vae.eval(), var.eval())
    return _MODELS[seed]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _source(prec='f32'):
    """the per-image call the tokens come from, computed once per precision and left unchanged"""
    if prec not in _SRC:
        vae, var = _model()
        var.set_hip_precision(prec)
        try:
            img, tok = var.autoregressive_infer_cfg_per_image(LABELS, SEEDS, cfg=CFG, return_tokens=True)
            _SRC[prec] = (img.clone(), tok.clone())
        finally:
            var.set_hip_precision('f32')
    return _SRC[prec]


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_the_same_label_gives_the_tokens_back_bit_for_bit(prec):
    vae, var = _model()
    img, tok = _source(prec)
    var.set_hip_precision(prec)
    try:
        r = var.counterfactual(tok, LABELS, LABELS, ABD_SEEDS, cfg=CFG)
    finally:
        var.set_hip_precision('f32')
    assert not bool(r.unreachable.any()) and bool(torch.isfinite(r.logp_src).all())
    assert torch.equal(r.tokens[:, 0], tok) and not bool(r.changed.any())
    assert r.first_changed_scale.tolist() == [[S]] * len(LABELS) and float(r.change_rate().abs().max()) == 0.0
    assert r.images.shape == (len(LABELS), 1) + tuple(img.shape[1:])
    err = float((r.images[:, 0] - img).abs().max())
    print(f'{prec}: max pixel difference to the per-image call {err:.3e}')
    assert err <= PIXEL[prec]
    # the source's log-probabilities are the replay's, the replay having drawn the same tokens from the same rows, up to the order of the
    # row sum (the sampler's W256 order here, rowlse.h's there): V roundings of the sum at worst, and a few of the logarithm and the difference
    u = 2.0 ** -24
    assert bool(((r.record.logp_guided - r.logp_src).abs() <= var.V * u + 4 * u * r.logp_src.abs()).all())
    assert r.noise.precision == prec and r.noise.noise.shape == (len(LABELS), var.L, var.V)


def test_another_label_keeps_the_scales_below_first_scale_and_first_scale_S_changes_nothing():
    vae, var = _model()
    _, tok = _source()
    free = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, decode=False)
    assert free.images is None and bool(free.changed.any())
    assert int(free.tokens.min()) >= 0 and int(free.tokens.max()) < var.V
    for first in (1, 3):
        r = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=first, decode=False)
        end = var.begin_ends[first - 1][1]
        assert torch.equal(r.tokens[:, 0, :end], tok[:, :end]) and bool((r.first_changed_scale >= first).all())
        assert bool(r.changed[:, 0, end:].any())
        assert bool(torch.isnan(r.record.logp_guided[:, :end]).all()) and bool(torch.isfinite(r.record.logp_guided[:, end:]).all())
        assert bool(torch.isnan(r.logp_src[:, :end]).all())
    r = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=S)
    assert torch.equal(r.tokens[:, 0], tok) and not bool(r.changed.any()) and r.first_changed_scale.tolist() == [[S]] * len(LABELS)
    assert r.images is not None and bool(torch.isfinite(r.images).all())


def test_a_request_does_not_depend_on_its_batch_its_column_or_the_chunking():
    vae, var = _model()
    _, tok = _source()
    kw = dict(decode=False, first_scale=1, top_k=[0, 900, 0, 600, 0, 50], top_p=[0.0, 0.96, 0.0, 0.5, 0.0, 0.9], cfg_dst=[1.5, 4.0, 0.0, 2.5, 3.0, 1.0])
    whole = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, **kw)
    sub = lambda x, idx: [x[i] for i in idx]
    def part(idx, dst=None, **over):
        k = dict(kw, **{key: sub(kw[key], idx) for key in ('top_k', 'top_p', 'cfg_dst')}, **over)
        return var.counterfactual(tok[idx], sub(LABELS, idx), sub(DST, idx) if dst is None else dst, sub(ABD_SEEDS, idx), cfg=sub(CFG, idx), **k)
    fields = lambda r, col=0: [r.tokens[:, col]] + [getattr(r.record, f).view(r.tokens.shape[0], r.tokens.shape[1], -1)[:, col] for f in r.record.FIELDS]
    same = lambda a, b: all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    for i in range(len(LABELS)):                                           # alone
        assert same(fields(part([i])), [f[i:i + 1] for f in fields(whole)]), i
    perm = [4, 2, 5, 0, 3, 1]                                              # a permuted batch
    assert same(fields(part(perm)), [f[perm] for f in fields(whole)])
    for idx in ([0], [1, 2], [3, 4, 5]):                                   # split 1 + 2 + 3
        assert same(fields(part(idx)), [f[idx] for f in fields(whole)]), idx
    assert same(fields(part(list(range(6)), max_images=1)), fields(whole))      # max_images = 1 equals max_images = 8
    # column k of a (B, K) call: K = 3 replays of one abduction, the middle column the request above
    dst3 = [[(d + 1) % 1001, d, (d + 500) % 1001] for d in DST]
    multi = var.counterfactual(tok, LABELS, dst3, ABD_SEEDS, cfg=CFG, max_images=4, **kw)
    assert multi.tokens.shape == (6, 3, var.L) and multi.first_changed_scale.shape == (6, 3)
    assert same(fields(multi, 1), fields(whole))
    assert not torch.equal(multi.tokens[:, 0], multi.tokens[:, 1])


def test_a_stored_record_replays_like_the_one_shot_call_and_foreign_records_are_refused():
    vae, var = _model()
    _, tok = _source()
    rec = var.abduct_noise(tok, LABELS, ABD_SEEDS, cfg=CFG, first_scale=1)
    assert rec.first_scale == 1 and rec.precision == 'f32' and rec.cfg == tuple(CFG) and rec.unreachable.dtype == torch.bool
    for first in (1, 2):                                                   # (a record serves every first_scale at or above its own)
        one = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=first)
        two = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=first, noise=rec)
        assert torch.equal(one.tokens, two.tokens) and torch.equal(_bits(one.images), _bits(two.images))
        assert torch.equal(_bits(one.record.logp_drawn), _bits(two.record.logp_drawn)) and two.noise is rec
    with pytest.raises(ValueError, match='first_scale'):
        var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=0, noise=rec)
    var.set_hip_precision('bf16')
    try:
        with pytest.raises(ValueError, match='f32'):
            var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=1, noise=rec)
    finally:
        var.set_hip_precision('f32')
    _, other = _model(seed=1)
    with pytest.raises(ValueError, match='other weights'):
        other.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=1, noise=rec)
    with pytest.raises(ValueError, match='NoiseRecord'):
        var.counterfactual(tok[:2], LABELS[:2], DST[:2], ABD_SEEDS[:2], cfg=CFG[:2], first_scale=1, noise=rec)
    with pytest.raises(ValueError):
        var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, first_scale=S + 1)
    with pytest.raises(TypeError):
        var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, more_smooth=True)
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        var.train().counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG)
    var.eval()


def test_target_top_k_1_is_the_greedy_sample_of_the_target():
    """top_k = 1 leaves the row's maximum alone (exact ties aside): the noise no longer matters, the replay is the target's greedy sequence"""
    vae, var = _model()
    _, tok = _source()
    r = var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, cfg_dst=2.0, top_k=1, decode=False)
    _, greedy = var.autoregressive_infer_cfg_per_image(DST, SEEDS, cfg=2.0, top_k=1, return_tokens=True)
    assert bool((r.record.kept == 1).all()), 'an exact tie at a maximum: the comparison below would not be defined'
    assert torch.equal(r.tokens[:, 0], greedy)


def test_the_models_generator_is_untouched_and_the_plain_call_unchanged():
    vae, var = _model()
    _, tok = _source()
    lab = torch.tensor(LABELS[:2], device='cuda')
    before = var.autoregressive_infer_cfg(2, lab, g_seed=4, cfg=1.5, top_k=900, top_p=0.96).clone()
    state = var.rng.get_state().clone()
    var.counterfactual(tok, LABELS, DST, ABD_SEEDS, cfg=CFG, max_images=4)
    assert torch.equal(var.rng.get_state(), state)
    after = var.autoregressive_infer_cfg(2, lab, g_seed=4, cfg=1.5, top_k=900, top_p=0.96)
    assert torch.equal(_bits(before), _bits(after))


def test_kept_scales_of_the_engines_sample_refuses_what_it_does_not_combine_with():
    vae, var = _model()
    _, tok = _source()
    eng, lab = var.engine(), torch.tensor(LABELS, device='cuda')
    B = len(LABELS)
    ok = dict(kept_scales=(tok, 2), decode=False)
    mask = torch.zeros(B, var.L, dtype=torch.bool, device='cuda')
    for bad in (dict(greedy=True), dict(more_smooth=True), dict(gt_tokens=tok, keep_mask=mask), dict(smooth=dict(gt=tok, n=4, thr=None)),
                dict(edit=dict(tokens=tok, mask=torch.ones(1, 4, 4, device='cuda')))):
        with pytest.raises(ValueError, match='kept_scales'):
            eng.sample(B, lab, var.rng, 1.5, 0, 0.0, **ok, **bad)
    for toks in (tok.int(), tok[:, :-1], tok[:2], tok.cpu()):
        with pytest.raises(ValueError, match='kept_scales tokens'):
            eng.sample(B, lab, var.rng, 1.5, 0, 0.0, kept_scales=(toks, 2), decode=False)
    out = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
    var.rng.manual_seed(3)
    eng.sample(B, lab, var.rng, 1.5, 0, 0.0, tokens_out=out, **ok)
    end = var.begin_ends[1][1]
    assert torch.equal(out[:, :end], tok[:, :end]) and int(out.min()) >= 0
