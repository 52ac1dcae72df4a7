"""VAR.sample_smc on the MI355X on the fixtures of tests/test_best_of_pruned_gpu.py: e2e_t_pn12345 (depth 2, 5 scales, L = 55;
boundaries behind scales 1 and 3) and d16_pn123 (3 scales, L = 14; a boundary behind scale 0).  No tolerances except the project's own bar
between the sampler's statistics and token_log_likelihood: without a resampling event the particles are the existing per-image calls bit for
bit, the fast route (device decision, caches resampled in place) equals the slow one (host twin, caches gathered out of place by torch), and an
image's result does not depend on its batch."""
import pytest
import torch

from tests.test_best_of_pruned_gpu import KW, REC, _bits, _model, _same_record
from tests.test_likelihood_gpu import kernel_bar_ok
from var_amd.models.var import SMCResult

pytestmark = pytest.mark.gpu

RESAMPLE = {'t_pn12345': (1, 3), 'd16_pn123': (0,)}
FIELDS = ('log_weights', 'ancestors', 'resampled', 'ess', 'log_weights_seen')


def _seeds(B, n, base=100):
    return [[base + 10 * b + c for c in range(n)] for b in range(B)]


def _same_smc(a: SMCResult, b: SMCResult, rows_a=slice(None), rows_b=slice(None), images=True):
    n = a.log_weights.shape[1]
    part = lambda r: r if r == slice(None) else slice(r.start * n, r.stop * n)
    _same_record(a.particles, b.particles, part(rows_a), part(rows_b))
    for k in FIELDS:
        assert torch.equal(_bits(getattr(a, k)[rows_a]), _bits(getattr(b, k)[rows_b])), k
    if images:
        assert (a.images is None) == (b.images is None) and (a.images is None or torch.equal(a.images[rows_a], b.images[rows_b]))


def _precision(var, prec):
    var.set_hip_precision(prec)


@pytest.mark.parametrize('name, prec', [('t_pn12345', 'f32'), ('t_pn12345', 'bf16'), ('d16_pn123', 'f32'), ('d16_pn123', 'bf16')])
def test_never_resampling_is_the_existing_calls(name, prec):
    var, lab = _model(name)
    seeds = _seeds(2, 4)
    _precision(var, prec)
    try:
        state = var.rng.get_state().clone()
        full = var.autoregressive_infer_cfg_per_image_scored(lab.repeat_interleave(4), [s for r in seeds for s in r], decode=False, **KW)
        img, win, totals, choice = var.sample_best_of(lab, seeds, by='logp_cond', **KW)
        zero = var.sample_smc(lab, seeds, resample=RESAMPLE[name], beta=0.0, decode=False, **KW)          # equal weights: ess == n
        none = var.sample_smc(lab, seeds, resample=(), beta=1.0, **KW)
        assert torch.equal(var.rng.get_state(), state), 'var.rng was read or advanced'
        for res in (zero, none):
            assert isinstance(res, SMCResult)
            _same_record(res.particles, full)
        K = len(RESAMPLE[name])
        assert not bool(zero.resampled.any()) and zero.resampled.shape == (2, K) and bool((zero.ess == 4.0).all())
        assert torch.equal(zero.ancestors, torch.arange(4, device='cuda').expand(2, K, 4)) and bool((zero.log_weights == 0).all())
        assert zero.images is None and zero.particles.images is None
        # resample=() at beta = 1: the weights are sample_best_of's totals, best() its choice, and the chosen particle's image its image
        assert none.ancestors.shape == (2, 0, 4) and none.resampled.shape == (2, 0)
        assert torch.equal(_bits(none.log_weights + 0.0), _bits(totals + 0.0)) and torch.equal(none.best(), choice)
        assert none.images.shape[:2] == (2, 4)
        one = var.sample_smc(lab, seeds, resample=(), beta=1.0, max_images=4, **KW)                       # the decoder's batch is sample_best_of's per image
        for b in range(2):
            own = var.autoregressive_infer_cfg_per_image_scored(lab[b:b + 1], [seeds[b][int(choice[b])]], **KW)
            assert torch.equal(one.particles.tokens[b * 4 + int(choice[b])], own.tokens[0])
    finally:
        _precision(var, 'f32')


@pytest.mark.parametrize('name, prec, n, beta', [('t_pn12345', 'f32', 4, 1.0), ('t_pn12345', 'f32', 8, 20.0), ('t_pn12345', 'bf16', 8, 1.0),
                                                 ('t_pn12345', 'bf16', 4, 20.0), ('d16_pn123', 'f32', 4, 20.0), ('d16_pn123', 'bf16', 8, 1.0)])
def test_fast_route_equals_slow_route_and_lineage(name, prec, n, beta):
    """3 images x n particles, ess=None (always resample).  The reference route takes its ancestors from the host twin and gathers the caches out
    of place; every field must be bit-equal, at least one slot must really have been overwritten, and every final particle's tokens through a
    boundary are, through `ancestors`, the tokens some slot held before that boundary"""
    var, lab2 = _model(name)
    lab = torch.cat((lab2, lab2[:1] + 1))
    seeds = _seeds(3, n)
    bounds = RESAMPLE[name]
    eng = var.engine()
    _precision(var, prec)
    try:
        fast = var.sample_smc(lab, seeds, resample=bounds, beta=beta, ess=None, **KW)
        eng.smc_reference = True
        try:
            slow = var.sample_smc(lab, seeds, resample=bounds, beta=beta, ess=None, **KW)
            pre = eng.smc_pre_tokens
        finally:
            eng.smc_reference = False
            eng.smc_pre_tokens = None
        _same_smc(fast, slow)
        assert bool(fast.resampled.all())
        ident = torch.arange(n, device='cuda').expand_as(fast.ancestors)
        moved = int((fast.ancestors != ident).sum())
        print(f'{name} {prec} n={n} beta={beta}: {moved} of {ident.numel()} slots overwritten, ess {fast.ess.tolist()}')
        assert moved >= 1, 'no slot was overwritten: the case shows nothing'
        anc = fast.ancestors
        assert torch.equal(anc.gather(2, anc), anc)
        # lineage: compose the later boundaries' tables; slot c's tokens below end(s_k) are the pre-boundary tokens of its ancestor at boundary k
        tok = fast.particles.tokens.view(3, n, -1)
        comp = torch.arange(n, device='cuda').expand(3, n)
        for k in reversed(range(len(bounds))):
            comp = anc[:, k].gather(1, comp)                          # the slot at boundary k whose (pre-boundary) state slot c descends from
            e = var.begin_ends[bounds[k]][1]
            assert pre[k].shape == (3, n, e)
            want = pre[k].gather(1, comp.view(3, n, 1).expand(3, n, e))
            assert torch.equal(tok[:, :, :e], want), f'boundary {k}'
    finally:
        _precision(var, 'f32')


@pytest.mark.parametrize('name', ['t_pn12345', 'd16_pn123'])
def test_the_caches_really_moved(name):
    """f32.  A copied particle's later tokens were drawn over its ancestor's K / V rows: token_log_likelihood on the final tokens (a teacher-forced
    pass that rebuilds every cache row from the tokens) must reproduce the statistics the sampler recorded.  Held to kernel_bar_ok
    (tests/test_likelihood_gpu.py), printed, and — measured on the MI355X: bit-equal on both fixtures, as DESIGN.md §26 observed for plain sampling —
    asserted equal."""
    var, lab = _model(name)
    n = 4
    res = var.sample_smc(lab, _seeds(2, n), resample=RESAMPLE[name], beta=20.0, ess=None, decode=False, **KW)
    assert int((res.ancestors != torch.arange(n, device='cuda').expand_as(res.ancestors)).sum()) >= 1
    tok = res.particles.tokens
    labs = lab.repeat_interleave(n)
    x = var.vae_proxy[0].quantize.idxBl_to_var_input([tok[:, b:e] for b, e in var.begin_ends])
    drop, var.cond_drop_rate = var.cond_drop_rate, 0.0
    try:
        with torch.no_grad():                                      # the rows' logits: kernel_bar_ok takes their magnitude
            cond, unc = var(labs, x), var(torch.full_like(labs, var.num_classes), x)
    finally:
        var.cond_drop_rate = drop
    S = len(var.patch_nums)
    t = torch.tensor([1.5 * (si / (S - 1)) for si, pn in enumerate(var.patch_nums) for _ in range(pn * pn)], device='cuda').view(1, -1, 1)
    for field, cfg, rows in (('logp_cond', 0.0, cond), ('logp_guided', 1.5, (1 + t) * cond - t * unc)):
        lp = var.token_log_likelihood(tok, labs.view(-1, 1), cfg=cfg)[:, 0]
        got = getattr(res.particles, field)
        ok, err = kernel_bar_ok(got, lp.double(), rows)
        print(f'{name} {field}: max |diff| to token_log_likelihood {err:.3e}, bit-equal: {torch.equal(_bits(lp), _bits(got))}')
        assert ok, f'{field} differs from token_log_likelihood by {err:.3e}'
        assert torch.equal(_bits(lp), _bits(got)), f'{field} is not token_log_likelihood bit for bit ({err:.3e})'      # observed on the MI355X on both fixtures


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_an_images_result_does_not_depend_on_its_batch(prec):
    var, lab2 = _model()
    lab = torch.cat((lab2, lab2[:1] + 1))
    n, bounds = 4, RESAMPLE['t_pn12345']
    seeds = _seeds(3, n)
    rs = [7, 8, 9]
    kw = dict(resample=bounds, beta=20.0, ess=None, n=n, decode=False, **KW)
    _precision(var, prec)
    try:
        whole = var.sample_smc(lab, seeds, resample_seeds=rs, max_images=64, **kw)
        for mi in (4, 8, 11):                                          # 1, 2 and 2 images per chunk
            _same_smc(whole, var.sample_smc(lab, seeds, resample_seeds=rs, max_images=mi, **kw))
        for b in range(3):                                             # alone
            one = var.sample_smc(lab[b:b + 1], seeds[b:b + 1], resample_seeds=rs[b:b + 1], **kw)
            _same_smc(whole, one, slice(b, b + 1), slice(0, 1))
        perm = [2, 0, 1]                                               # another position, the same resample_seeds entry
        moved = var.sample_smc(lab[perm], [seeds[p] for p in perm], resample_seeds=[rs[p] for p in perm], **kw)
        for i, p in enumerate(perm):
            _same_smc(whole, moved, slice(p, p + 1), slice(i, i + 1))
        # the default key is the image's first seed
        _same_smc(var.sample_smc(lab, seeds, **kw), var.sample_smc(lab, seeds, resample_seeds=[r[0] for r in seeds], **kw))
    finally:
        _precision(var, 'f32')


def test_no_second_cache_set():
    var, lab = _model(fresh=True)                            # (no buffer set of an earlier test)
    seeds = _seeds(2, 4)
    eng = var.engine()
    kw = dict(n=4, by='logp_cond', decode=False, **KW)
    var.sample_best_of_pruned(lab, seeds, None, **kw)
    first = var.sample_smc(lab, seeds, resample=(1, 3), beta=20.0, ess=None, **kw)
    sets = {k: [t.data_ptr() for t in v['kc'] + v['vc']] for k, v in eng._ws_bop.items()}
    assert len(sets) == 1, 'sample_smc holds more than one cache set'
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    res = var.sample_best_of_pruned(lab, seeds, None, **kw)
    torch.cuda.synchronize(); peak_bop = torch.cuda.max_memory_allocated() - base
    del res
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    again = var.sample_smc(lab, seeds, resample=(1, 3), beta=20.0, ess=None, **kw)
    torch.cuda.synchronize(); peak_smc = torch.cuda.max_memory_allocated() - base
    assert {k: [t.data_ptr() for t in v['kc'] + v['vc']] for k, v in eng._ws_bop.items()} == sets, 'a repeated call allocated cache memory'
    _same_smc(first, again)
    nbytes = lambda t: 0 if t is None else t.numel() * t.element_size()
    result = sum(nbytes(getattr(again, k)) for k in FIELDS + ('images',)) + sum(nbytes(getattr(again.particles, k)) for k in REC)
    cache_set = sum(nbytes(t) for v in eng._ws_bop.values() for t in v['kc'] + v['vc'])
    print(f'peak above the resident state: sample_smc {peak_smc} B, sample_best_of_pruned(keep=None) {peak_bop} B, result tensors {result} B, one cache set {cache_set} B')
    assert peak_smc <= peak_bop + result


def test_refusals():
    var, lab = _model()
    seeds = _seeds(2, 4)
    for bad in ((4,), (5,), (3, 1), (1, 1), (-1,), (True,), (1.0,), 'ab', None, {1: 2}, 3):
        with pytest.raises(ValueError, match='resample'):
            var.sample_smc(lab, seeds, resample=bad, **KW)
    for bad in (0, 0.0, -0.5, 1.5, float('nan'), True, 'x'):
        with pytest.raises(ValueError, match='ess'):
            var.sample_smc(lab, seeds, resample=(1,), ess=bad, **KW)
    for bad in (dict(by='entropy'), dict(by='kept'), dict(n=2), dict(max_images=0), dict(beta=float('inf')), dict(resample_seeds=[1]), dict(resample_seeds=[1, -2])):
        with pytest.raises(ValueError):
            var.sample_smc(lab, seeds, resample=(1,), **dict(KW, **bad))
    with pytest.raises(ValueError, match='max_images'):
        var.sample_smc(lab, seeds, resample=(1,), max_images=3, **KW)
    with pytest.raises(TypeError):
        var.sample_smc(lab, seeds, resample=(1,), more_smooth=True, **KW)
    import contextlib
    import io
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        _, cpu = build_vae_var(device='cpu', patch_nums=(1, 2, 3), depth=2, ch=32)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cpu.eval().sample_smc(lab.cpu(), seeds, resample=(1,), **KW)


@pytest.mark.parametrize('bounds, max_images', [((1, 3), 8), ((1, 3), 4), ((), 8), ((0,), 64), ((0, 1, 2, 3), 8)])
def test_smc_work_is_what_the_schedule_implies(bounds, max_images):
    var, lab = _model()
    var.sample_smc(lab, _seeds(2, 4), resample=bounds, decode=False, max_images=max_images, **KW)
    be, S = var.begin_ends, len(var.patch_nums)
    want, first = [], 0
    for s in list(bounds) + [S - 1]:
        want.append((s, 2 * 4 * (be[s][1] - be[first][0])))
        first = s + 1
    assert var.engine().smc_work == want
