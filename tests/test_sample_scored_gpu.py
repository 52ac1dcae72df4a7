"""Scored sampling on the MI355X: VAR.autoregressive_infer_cfg_scored, ..._per_image_scored and sample_best_of on the
fixtures e2e_t_pn12345 (depth 2) and d16_pn123, B <= 4: images and tokens bit-equal to the plain calls, no trace left in the RNG stream or
the workspaces, every field against float64 on the traced logits and against VAR.token_log_likelihood, batch independence, best-of-n."""
import numpy as np
import pytest
import torch

from tests import samplestatsref as R
from tests import util
from tests.test_e2e_gpu import build_models
from tests.test_likelihood_gpu import kernel_bar_ok
from var_amd.models.var import SampleRecord, rule_order

pytestmark = pytest.mark.gpu

KW = dict(cfg=1.5, top_k=900, top_p=0.96)
REC = ('tokens',) + SampleRecord.FIELDS


def _model(name='t_pn12345'):
    z, meta = util.load_case(name)
    vae, var = build_models(meta)
    return var, torch.tensor(meta['labels'], dtype=torch.int64, device='cuda')


def _same(a: SampleRecord, b: SampleRecord, rows_a=slice(None), rows_b=slice(None)):
    """every per-token field bit for bit (NaN-free here: torch.equal on the int32 views)"""
    for k in REC:
        x, y = getattr(a, k)[rows_a], getattr(b, k)[rows_b]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), k


@pytest.mark.parametrize('name, prec, more_smooth', [('t_pn12345', 'f32', False), ('t_pn12345', 'f16', False), ('t_pn12345', 'f32', True),
                                                      ('t_pn12345', 'f16', True), ('d16_pn123', 'f32', False), ('d16_pn123', 'bf16', False)])
def test_scored_call_is_the_plain_call(name, prec, more_smooth):
    """images and tokens bit-equal to autoregressive_infer_cfg with the same seed; a plain call issued after a scored call gives what it gives
    after a plain call (RNG stream, workspaces)"""
    var, lab = _model(name)
    var.set_hip_precision(prec)
    try:
        B = lab.numel()
        eng = var.engine()
        more = lambda **kw: eng.sample(B, lab, var.rng, KW['cfg'], KW['top_k'], KW['top_p'], more_smooth=more_smooth, **kw).clone()   # continues var.rng's stream
        tok = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
        var.rng.manual_seed(7)
        more(tokens_out=tok)
        plain = var.autoregressive_infer_cfg(B, lab, g_seed=7, more_smooth=more_smooth, **KW).clone()
        after_plain = more()
        rec = var.autoregressive_infer_cfg_scored(B, lab, g_seed=7, more_smooth=more_smooth, **KW)
        after_scored = more()
        assert torch.equal(rec.images, plain), 'the scored call changed the images'
        assert torch.equal(rec.tokens, tok), 'the scored call changed the tokens'
        assert torch.equal(after_scored, after_plain), 'a plain call differs after a scored call'
        assert rec.patch_nums == tuple(var.patch_nums) and rec.kept.dtype == torch.int32 and rec.logp_cond.shape == (B, var.L)
        assert bool((rec.kept >= 1).all()) and bool((rec.kept <= 900).all()) and bool(torch.isfinite(rec.entropy).all())
        assert bool((rec.logp_drawn <= 0).all()) and bool(torch.isfinite(rec.logp_drawn).all())
        nod = var.autoregressive_infer_cfg_scored(B, lab, g_seed=7, more_smooth=more_smooth, decode=False, **KW)
        assert nod.images is None
        _same(nod, rec)
        ps = rec.per_scale()
        assert ps['logp_cond'].shape == (B, len(var.patch_nums)) and ps['kept'].dtype == torch.float64 and 'SampleRecord(B=' in repr(rec)
        want = np.add.accumulate(rec.logp_guided.double().cpu().numpy(), axis=1)[:, -1]
        assert np.array_equal(rec.total('logp_guided').numpy(), want)
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('name, prec', [('t_pn12345', 'f32'), ('t_pn12345', 'f16'), ('d16_pn123', 'f32'), ('d16_pn123', 'auto')])
def test_fields_against_float64_on_the_traced_logits(name, prec):
    """sample(trace=True, stats=...): every field within the derived bounds (tests/samplestatsref.py) of float64 on the per-scale logits the
    head wrote (fp32 in every precision: one kernel)"""
    var, lab = _model(name)
    var.set_hip_precision(prec)
    ctx = torch.autocast('cuda', dtype=torch.float16) if prec == 'auto' else torch.autocast('cuda', enabled=False)
    try:
        B, V, S = lab.numel(), var.V, len(var.patch_nums)
        for top_k, top_p in ((900, 0.96), (0, 0.0)):
            st = {}
            with ctx:
                var.rng.manual_seed(3)
                var.engine().sample(B, lab, var.rng, 1.5, top_k, top_p, trace=True, stats=st)
            tr = var.engine().last_trace
            for si, ((b0, e0), pn) in enumerate(zip(var.begin_ends, var.patch_nums)):
                l, t = pn * pn, 1.5 * (si / (S - 1))
                logits = tr['logits'][si].reshape(2 * B * l, V).cpu().numpy()
                idx = tr['idx'][si].reshape(-1).cpu().numpy()
                z = R.guided_rows(logits, B, l, t)
                got = {k: st[f].cpu().numpy()[:, b0:e0] for k, f in (('lp_cond', 'logp_cond'), ('lp_guided', 'logp_guided'), ('lp_drawn', 'logp_drawn'),
                                                                    ('kept', 'kept'), ('entropy', 'entropy'))}
                masked = tr['masked'][si].cpu().numpy()                 # the sampler's filtered logits of the scale (traced with stats)
                if top_k == 0:                                          # nothing filtered: the drawn distribution is the guided one
                    assert np.array_equal(masked.view(np.uint32), z.view(np.uint32))
                    assert np.array_equal(got['lp_drawn'].view(np.uint32), got['lp_guided'].view(np.uint32)) and (got['kept'] == V).all()
                else:
                    assert (got['kept'] <= 900).all() and (got['kept'] >= 1).all()
                ref = R.reference(logits, masked, idx, B, l, t)
                slack = R.lp_bound(ref['lp_drawn'], V) + R.lp_bound(ref['lp_guided'], V)
                assert (got['lp_drawn'] >= got['lp_guided'] - slack).all()
                R.check_against_reference(got, ref, V, f'{name} {prec} scale {si}: ')
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('name', ['t_pn12345', 'd16_pn123'])
def test_fields_agree_with_token_log_likelihood(name):
    """logp_cond against token_log_likelihood(tokens, label, cfg=0), logp_guided against the same call at the same cfg.  Measured on the MI355X
    in f32: bit-equal on both fixtures (the teacher-forced pass rebuilds the same logits bit for bit in its own batch layout, and the row
    code is one piece), so that is what is asserted, in place of the bar tests/test_likelihood_gpu.py holds between its two
    routes (kernel_bar_ok, test_likelihood_gpu.py:21-25: 1e-6 (|lp| + max|z| + 8), still evaluated and printed).  For logp_guided the
    equality needs the two guidance factors to agree: the scorer rounds cfg * si / (S - 1) in fp32, the sampler in float64; with S = 3 and
    S = 5 every ratio is exact in both, so they do on these fixtures."""
    var, lab = _model(name)
    B, V = lab.numel(), var.V
    st = {}
    tok = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
    var.rng.manual_seed(5)
    var.engine().sample(B, lab, var.rng, 1.5, 900, 0.96, trace=True, stats=st, tokens_out=tok)
    tr = var.engine().last_trace
    S = len(var.patch_nums)
    cond = torch.cat([x[:B] for x in tr['logits']], dim=1)                                  # (B, L, V)
    unc = torch.cat([x[B:] for x in tr['logits']], dim=1)
    t = torch.tensor([1.5 * (si / (S - 1)) for si, pn in enumerate(var.patch_nums) for _ in range(pn * pn)], device='cuda').view(1, -1, 1)
    z = (1 + t) * cond - t * unc
    for field, cfg, rows in (('logp_cond', 0.0, cond), ('logp_guided', 1.5, z)):
        lp = var.token_log_likelihood(tok, lab.view(B, 1), cfg=cfg)[:, 0]
        ok, err = kernel_bar_ok(st[field], lp.double(), rows)
        print(f'{name} {field}: max |diff| to token_log_likelihood {err:.3e} (bar ok: {ok})')
        assert torch.equal(lp.view(torch.int32), st[field].view(torch.int32)), f'{field} is not token_log_likelihood bit for bit ({err:.3e})'


@pytest.mark.parametrize('name, prec, more_smooth', [('t_pn12345', 'f32', False), ('t_pn12345', 'bf16', True), ('d16_pn123', 'f32', False)])
def test_per_image_record_does_not_depend_on_the_batch(name, prec, more_smooth):
    """four requests in one batch and each alone: tokens and every per-token field bit-equal; tokens and images equal the unscored per-image call"""
    var, _ = _model(name)
    var.set_hip_precision(prec)
    try:
        labs, seeds, cfgs, ks, ps = [3, 980, 1000, 417], [17, 3, (1 << 62) + 5, 0], [4.0, 1.5, 0.0, 2.5], [0, 900, 1, 600], [0.96, 0.0, 0.0, 0.5]
        rec = var.autoregressive_infer_cfg_per_image_scored(labs, seeds, cfg=cfgs, top_k=ks, top_p=ps, more_smooth=more_smooth)
        img, tok = var.autoregressive_infer_cfg_per_image(labs, seeds, cfg=cfgs, top_k=ks, top_p=ps, more_smooth=more_smooth, return_tokens=True)
        assert torch.equal(rec.images, img) and torch.equal(rec.tokens, tok)
        assert bool((rec.kept[2] == 1).all()) and bool((rec.logp_drawn[2] == 0).all())          # top_k = 1
        assert bool((rec.kept[0] <= var.V).all()) and bool((rec.kept[3] <= 600).all())
        for b in range(4):
            one = var.autoregressive_infer_cfg_per_image_scored(labs[b:b + 1], seeds[b:b + 1], cfg=cfgs[b], top_k=ks[b], top_p=ps[b],
                                                                more_smooth=more_smooth, decode=False)
            _same(rec, one, slice(b, b + 1))
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('name', ['t_pn12345', 'd16_pn123'])
@pytest.mark.parametrize('by', ['logp_cond', 'logp_drawn'])
def test_best_of(name, by):
    """B = 2, n = 3: choice is the rule applied on the host to totals; totals are the candidates' own sums; a winner's image and record are those
    of autoregressive_infer_cfg_per_image_scored with that candidate's seed alone; chunking changes nothing"""
    var, lab = _model(name)
    seeds = [[11, 12, 13], [21, 22, 23]]
    img, win, totals, choice = var.sample_best_of(lab, seeds, n=3, by=by, **KW)
    assert img.shape[0] == 2 and totals.shape == (2, 3) and totals.dtype == torch.float64 and choice.dtype == torch.int64
    tot = totals.cpu().numpy()
    assert [int(rule_order(tot[b])[0]) for b in range(2)] == choice.tolist()
    assert torch.equal(win.images, img)
    for b in range(2):
        for c in range(3):
            one = var.autoregressive_infer_cfg_per_image_scored(lab[b:b + 1], [seeds[b][c]], decode=(c == choice[b].item()), **KW)
            assert float(one.total(by)[0]) == tot[b, c], (b, c)
            if c == choice[b].item():
                _same(win, one, slice(b, b + 1))
                assert torch.equal(one.images[0], img[b]), f'image {b}: the winner differs from its own per-image call'
    img2, win2, totals2, choice2 = var.sample_best_of(lab, torch.tensor(seeds), by=by, max_images=2, **KW)
    assert torch.equal(img2, img) and torch.equal(totals2, totals) and torch.equal(choice2, choice)
    _same(win2, win)


def test_best_of_one_is_the_per_image_call():
    var, lab = _model()
    img, win, totals, choice = var.sample_best_of(lab, [[5], [6]], **KW)
    rec = var.autoregressive_infer_cfg_per_image_scored(lab, [5, 6], **KW)
    assert choice.tolist() == [0, 0] and torch.equal(img, rec.images) and torch.equal(totals[:, 0].cpu(), rec.total('logp_cond'))
    _same(win, rec)


def test_refused_combinations_and_cpu_model():
    var, lab = _model()
    eng, B = var.engine(), lab.numel()
    gt = torch.zeros(B, var.L, dtype=torch.int64, device='cuda')
    keep = torch.zeros(B, var.L, dtype=torch.bool, device='cuda')
    for bad in (dict(greedy=True), dict(smooth=dict(gt=gt, n=4, thr=None)), dict(gt_tokens=gt, keep_mask=keep),
                dict(edit=dict(tokens=gt, mask=torch.ones(1, 5, 5, device='cuda')))):
        with pytest.raises(ValueError):
            eng.sample(B, lab, None, 1.5, 0, 0.0, stats={}, **bad)
    with pytest.raises(ValueError):
        eng.sample(B, lab, None, 1.5, 0, 0.0, stats=dict(kept=torch.zeros(B, var.L, device='cuda')))      # wrong dtype
    for bad in (dict(by='entropy'), dict(n=2), dict(max_images=0)):
        with pytest.raises(ValueError):
            var.sample_best_of(lab, [[1, 2, 3], [4, 5, 6]], **bad)
    with pytest.raises(ValueError):
        var.sample_best_of(lab, [1, 2])
    from models import build_vae_var
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        _, cpu = build_vae_var(device='cpu', patch_nums=(1, 2), depth=2, ch=32)
    cpu.eval()
    for call in (lambda: cpu.autoregressive_infer_cfg_scored(1, 3), lambda: cpu.autoregressive_infer_cfg_per_image_scored([3], [1]),
                 lambda: cpu.sample_best_of([3], [[1, 2]])):
        with pytest.raises(RuntimeError, match='HIP kernels only'):
            call()
