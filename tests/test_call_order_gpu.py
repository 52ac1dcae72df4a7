"""History independence of the engines on a real MI355X: the result of a public call depends on the weights, the arguments,
the seed and the precision, never on what the model object did before.

A fixed deck of 103 calls (sampling at several batch sizes, editing, inpainting, smooth sampling, the teacher-forced forward, the scoring and
classification calls, per-image and scored sampling, best-of-n, evaluate, the distance / class-information / attention profiles, the class heat
maps, the VQVAE's own entry points with VQVAE.forward, four calls that are refused on the host; every call that has 16-bit modes in f32, f16
and bf16, one under 'auto' inside an autocast region) is run
  alone        each entry as the FIRST call on a model nothing has touched; where a fixture under tests/golden pins the call, its tokens are
               asserted against the reference's, so "alone" is anchored to the reference and not only to itself; the scored calls are anchored
               to the calls they extend;
  in company   on ONE model per configuration that is never rebuilt: the deck in its listed order, reversed, and in three seeded permutations;
  poisoned     one more pass, with every tensor the engines keep between calls that is not a copy of the weights overwritten before each call
               (0xFF bytes: NaN in every float format, 255 in uint8 maps; V - 1, a legal index, in integer buffers) and a NaN-filled block
               handed back to the allocator.  A walk over the live engine objects asserts that this is every such tensor.
Every result must equal the entry's alone result BIT FOR BIT (the fp32 path is under a bit-exactness contract, the 16-bit kernels are asserted
run-to-run deterministic, 'auto' is asserted bit-equal to the explicit modes: no tolerance is needed or used).

Then: workspaces across eight batch sizes, two streams in flight and a precision switch; the teacher-forcing workspaces across nine row counts,
two streams in flight and a precision switch; a parameter replaced by a new one that lands on the old one's address with the old one's
version counter, and one whose storage the engine holds beside tables derived from it; the label range check against a recycled address
(through _check_labels alone: no kernel ever sees the bad label).  Every call in this file is a legal call, or one the host refuses before
any launch.  One anchor is toleranced: `vae_forward_d_b3` is held to the reference's fixture within the bounds that
tests/test_vae_forward_gpu.py uses against the same fixture (REC_ATOL, LOSS_REL_BOUND), as `forward_eval` is held to its fixture; no comparison
between two runs of this project has a tolerance."""
import collections
import contextlib
import gc
import json
import os

import numpy as np
import pytest

from tests import util
from tests import test_e2e_gpu as e2e

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PRECS = ('f32', 'f16', 'bf16')
SCORE_LABELS = [980, 437, 3, 1000, 7, 512]          # 1000 == num_classes: the unconditional class is a legal label

Entry = collections.namedtuple('Entry', 'name model policy autocast fn anchor raises')
_FIX, _ALONE, _COMPANY = {}, {}, {}


# ---- fixtures and models ---------------------------------------------------------------------------------------------------------------
def fix(name):
    if name not in _FIX:
        z = np.load(os.path.join(util.GOLD, name + '.npz'))
        _FIX[name] = (z, json.loads(str(z['meta'])))
    return _FIX[name]


def model_meta(kind):
    return fix('e2e_t_pn12345' if kind == 't' else 'e2e_d16_pn123')[1]


def fresh(kind):
    """a model no call has touched, built the way tests/test_e2e_gpu.py::build_models builds it and taken out of that file's cache"""
    e2e._MODELS.clear()
    vae, var = e2e.build_models(model_meta(kind))
    e2e._MODELS.clear()
    var.cond_drop_rate = 0.0                  # VAR.forward drops labels at random otherwise (var.py:200), also in eval
    return vae, var


def company(kind):
    """the one model of a configuration that every in-company pass of this file shares: built once, never rebuilt"""
    if kind not in _COMPANY:
        _COMPANY[kind] = fresh(kind)
    return _COMPANY[kind]


def cuda_i64(a):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).cuda()


def labels_of(B):
    return [(91 * i + 7) % 1001 for i in range(B)]


# ---- the deck --------------------------------------------------------------------------------------------------------------------------
def ar(B, seed, more_smooth=False):
    def fn(vae, var):
        lab = torch.tensor(labels_of(B), device='cuda')
        return dict(img=var.autoregressive_infer_cfg(B, lab, g_seed=seed, cfg=1.5, top_k=900, top_p=0.96, more_smooth=more_smooth))
    return fn


def e2e_fixture(case):
    """the reference's own run (its Exp(1) stream injected) as tests/test_e2e_gpu.py::hip_run makes it"""
    def fn(vae, var):
        z, meta = fix('e2e_' + case)
        noise = [torch.from_numpy(n) for n in util.regen_noise(meta, z)]
        lab = torch.tensor(meta['labels'], dtype=torch.int64, device='cuda')
        eng = var.engine()
        img = eng.sample(len(meta['labels']), lab, None, meta['cfg'], meta['top_k'], meta['top_p'], noises=noise, trace=True)
        tr = eng.last_trace
        return dict(img=img, idx=torch.cat(tr['idx'], 1), logits=torch.cat(tr['logits'], 1), f_hat=tr['f_hat'][-1], pooled=torch.cat([p.flatten(2) for p in tr['pooled']], 2))

    def anchor(res):
        z, _ = fix('e2e_' + case)
        assert np.array_equal(res['idx'].numpy().astype(np.int32), z['idx']), f'{case}: tokens differ from the reference fixture'
    return fn, anchor


def edit_public(vae, var):
    z, meta = fix('edit_a_inpaint')
    lab = torch.tensor(meta['labels'], device='cuda')
    img = var.autoregressive_infer_cfg_with_mask(meta['B'], lab, g_seed=1, cfg=meta['cfg'], top_k=meta['top_k'], top_p=meta['top_p'],
                                                 input_img_tokens=torch.from_numpy(z['tokens'].astype(np.int64)), edit_mask=torch.from_numpy(z['mask']))
    return dict(img=img)


def edit_fixture(vae, var):
    from tests.test_edit_gpu import regen_edit_noise
    z, meta = fix('edit_a_inpaint')
    n1, n2 = regen_edit_noise(meta, z)
    lab = torch.tensor(meta['labels'], device='cuda')
    out = torch.empty(meta['B'], var.L, dtype=torch.int64, device='cuda')
    eng = var.engine()
    img = eng.sample(meta['B'], lab, None, meta['cfg'], meta['top_k'], meta['top_p'], noises=n1, gumbel_noises=n2, more_smooth=meta['more_smooth'],
                     trace=True, tokens_out=out, edit=dict(tokens=cuda_i64(z['tokens']), mask=torch.from_numpy(z['mask']).cuda()))
    return dict(img=img, final=out, f_hat=eng.last_trace['f_hat'][-1])


def edit_anchor(res):
    z, _ = fix('edit_a_inpaint')
    assert np.array_equal(res['final'].numpy().astype(np.int32), z['final']), 'edit_a_inpaint: final tokens differ from the reference fixture'


def inpaint_public(vae, var):
    z, meta = fix('inpaint_t_pn12345')
    lab = torch.tensor(meta['labels'], device='cuda')
    return dict(img=var.inpainting(cuda_i64(z['gt']), torch.from_numpy(z['mask']).cuda(), label=lab, g_seed=3, cfg=meta['cfg'], top_k=meta['top_k'],
                                   top_p=meta['top_p']))


def inpaint_fixture(vae, var):
    from tests.test_oracle_vs_golden import regen_inpaint_noise
    z, meta = fix('inpaint_t_pn12345')
    noise = [torch.from_numpy(n) for n in regen_inpaint_noise(meta, z)]
    lab = torch.tensor(meta['labels'], device='cuda')
    eng = var.engine()
    img = eng.sample(len(meta['labels']), lab, None, meta['cfg'], meta['top_k'], meta['top_p'], noises=noise, trace=True,
                     gt_tokens=cuda_i64(z['gt']), keep_mask=torch.from_numpy(z['mask']).cuda())
    return dict(img=img, idx=torch.cat(eng.last_trace['idx'], 1), f_hat=eng.last_trace['f_hat'][-1])


def inpaint_anchor(res):
    z, _ = fix('inpaint_t_pn12345')
    assert np.array_equal(res['idx'].numpy().astype(np.int32), z['idx']), 'inpaint_t_pn12345: tokens differ from the reference fixture'


def smooth(case):
    """VAR.smooth_sampling with the fixture's arguments (no sampler and, without more_smooth, no RNG draw: the engine call below is the public
    call with the chosen tokens traced)"""
    def fn(vae, var):
        z, meta = fix(case)
        lab = torch.tensor(meta['labels'], device='cuda')
        eng = var.engine()
        img = eng.sample(len(meta['labels']), lab, None, meta['cfg'], 0, 0.0, trace=True, more_smooth=False,
                         smooth=dict(gt=cuda_i64(z['gt']), n=meta['n'], thr=meta['thr']))
        return dict(img=img, idx=torch.cat(eng.last_trace['idx'], 1), sum_ll=eng.last_smooth[0], sum_dist_ll=eng.last_smooth[1])

    def anchor(res):
        z, _ = fix(case)
        assert np.array_equal(res['idx'].numpy().astype(np.int32), z['idx']), f'{case}: tokens differ from the reference fixture'
    return fn, anchor


def forward_eval(vae, var):
    z, meta = fix('encode_t_pn12345')
    assert not var.training
    return dict(logits=var(torch.tensor(meta['labels'], device='cuda'), torch.from_numpy(z['var_input']).cuda()))


def forward_anchor(res):
    z, _ = fix('encode_t_pn12345')
    ok, m = util.diff_report('teacher-forced logits vs reference', res['logits'].numpy(), z['logits'], atol=3e-4, rtol=1e-5)
    assert ok, m


def scoring_gt():
    return cuda_i64(fix('inpaint_t_pn12345')[0]['gt'])


def loglik(vae, var):
    return dict(lp=var.token_log_likelihood(scoring_gt(), torch.tensor(SCORE_LABELS), cfg=1.5, max_rows=8))


def scores(mode, **kw):
    def fn(vae, var):
        return dict(s=var.token_scores(scoring_gt(), torch.tensor(SCORE_LABELS), mode, cfg=1.5, max_rows=5, **kw))
    return fn


def classify(vae, var):
    r = var.classify(scoring_gt(), torch.tensor(SCORE_LABELS), 'log_prob', cfg=1.5, max_rows=8, keep={1: 3, 2: 2})
    return dict(pred=r.pred, total=r.total, depth=r.depth, tokens=r.tokens)


def generative(feat):
    def fn(vae, var):
        z, _ = fix('generative_t_pn12345')
        r = var.classify_generative(torch.from_numpy(z['img']).cuda(), torch.from_numpy(z['labels']), 1, feat, cfg=4.0)
        return dict(pred=r.pred, score=r.score, tokens=r.tokens)

    def anchor(res):
        z, _ = fix('generative_t_pn12345')
        assert np.array_equal(res['tokens'].numpy(), z[f'{feat}_cfg4_c1_tokens'].astype(np.int64)), f'generative {feat}: tokens differ from the reference fixture'
    return fn, anchor


def vae_encode(vae, var):
    z, _ = fix('encode_t_pn12345')
    idx = vae.img_to_idxBl(torch.from_numpy(z['img']).cuda())
    return {f's{si}': i for si, i in enumerate(idx)}


def vae_encode_anchor(res):
    z, meta = fix('encode_t_pn12345')
    for si in range(len(meta['patch_nums'])):
        assert np.array_equal(res[f's{si}'].numpy().astype(np.int32), z[f'idx_s{si}']), f'img_to_idxBl scale {si}: tokens differ from the reference fixture'


def vae_decode_fhat(vae, var):
    z, _ = fix('encode_t_pn12345')
    return dict(img=vae.fhat_to_img(torch.from_numpy(z['f_hat_last']).cuda()))


def vae_decode_tokens(vae, var):
    z, meta = fix('encode_t_pn12345')
    return dict(img=vae.idxBl_to_img([cuda_i64(z[f'idx_s{si}']) for si in range(len(meta['patch_nums']))], same_shape=True, last_one=True))


def encoder_blocks_leave_partials(vae, var):
    """the encoder engine's building blocks, used as the engine uses them: a conv leaves GroupNorm partials for ITS result; a gn() of another map
    of the same shape must compute that map's own statistics.  The entry ends with partials pending, for a map the size of conv_in's result
    at this batch size: the next encode on this model must not take them for its own."""
    enc = vae._encoder_engine()
    enc.refresh(); enc._wait_ready()
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(2, 80, 80, 32, generator=g).cuda(), torch.randn(2, 80, 80, 32, generator=g).cuda()
    pre = 'encoder.down.0.block.0'
    enc._gn_part = None
    want = enc.gn(b, pre + '.norm2', 2, 6400, True)
    out = enc.conv3(a, pre + '.conv1', 2, 80, 80, stats=True)
    assert enc._gn_part is not None and enc._gn_part[0] is out
    got = enc.gn(b, pre + '.norm2', 2, 6400, True)
    assert enc._gn_part is None                                   # (got == want is asserted on the alone result and compared in every pass)
    own = enc.gn(out, pre + '.norm2', 2, 6400, True)             # (no partials pending: the statistics pass)
    out2 = enc.conv3(a, pre + '.conv1', 2, 80, 80, stats=True)
    own2 = enc.gn(out2, pre + '.norm2', 2, 6400, True)            # (from the partials)
    enc.conv3(a, pre + '.conv1', 2, 80, 80, stats=True)           # left pending
    return dict(out=out, gn_other=got, gn_other_want=want, gn_own_full=own, gn_own_part=own2)


def bad_labels(vae, var):
    var.autoregressive_infer_cfg(2, torch.tensor([5, 1001], device='cuda'), g_seed=1, cfg=1.5, top_k=900, top_p=0.96)


def bad_gt_length(vae, var):
    var.token_log_likelihood(scoring_gt()[:, :-1], torch.tensor(SCORE_LABELS), cfg=1.5, max_rows=8)


def bad_score(vae, var):
    var.token_scores(scoring_gt(), torch.tensor(SCORE_LABELS), 'entropy', cfg=1.5, max_rows=8)


# ---- the calls added after the deck was first written: per-image and scored sampling, best-of-n, the teacher-forced metrics and maps,
# VQVAE.forward (each result object is flattened into its tensor fields, every one of them)
PER_IMAGE = dict(seeds=[101, 7, (1 << 40) + 3], cfg=[1.5, 0.0, 4.0], top_k=[900, 0, 50], top_p=[0.96, 0.0, 0.5])


def record_fields(r, pre=''):
    out = {pre + k: getattr(r, k) for k in ('tokens',) + r.FIELDS}
    if r.images is not None:
        out[pre + 'images'] = r.images
    return out


def per_image(vae, var):
    p = PER_IMAGE
    img, tok = var.autoregressive_infer_cfg_per_image(torch.tensor(labels_of(3)), p['seeds'], cfg=p['cfg'], top_k=p['top_k'], top_p=p['top_p'], return_tokens=True)
    return dict(img=img, tokens=tok)


def per_image_more_smooth(vae, var):
    return dict(img=var.autoregressive_infer_cfg_per_image(torch.tensor(labels_of(2)), [31, 32], cfg=1.5, top_k=900, top_p=0.96, more_smooth=True))


def per_image_d16(vae, var):
    img, tok = var.autoregressive_infer_cfg_per_image(torch.tensor(labels_of(5)), [41, 42, 43, 44, 45], cfg=[1.5, 3.0, 0.0, 1.5, 2.0], top_k=900, top_p=0.96,
                                                      return_tokens=True)
    return dict(img=img, tokens=tok)


def ar_scored(vae, var):
    lab = torch.tensor(labels_of(2), device='cuda')
    return record_fields(var.autoregressive_infer_cfg_scored(2, lab, g_seed=11, cfg=1.5, top_k=900, top_p=0.96))


def per_image_scored(vae, var):
    p = PER_IMAGE
    return record_fields(var.autoregressive_infer_cfg_per_image_scored(torch.tensor(labels_of(3)), p['seeds'], cfg=p['cfg'], top_k=p['top_k'], top_p=p['top_p']))


def best_of(vae, var):
    """six candidates in chunks of four: 4 + 2, so the second chunk samples at another batch size over the first one's buffers"""
    img, win, totals, choice = var.sample_best_of(torch.tensor(labels_of(2)), [[51, 52, 53], [61, 62, 63]], n=3, by='logp_drawn', cfg=[1.5, 3.0], top_k=900,
                                                  top_p=0.96, max_images=4)
    return dict(img=img, totals=totals, choice=choice, **record_fields(win, 'win_'))


def eval_tokens(N, L, V=4096):
    """N legal token rows of length L: the scoring fixture's two rows where they fit, continued by a fixed affine walk over the vocabulary"""
    base = scoring_gt().cpu()
    if L != base.shape[1]:
        base = (torch.arange(2 * L).view(2, L) * 977 + 131) % V
    return torch.stack([(base[i % 2] * (2 * (i // 2) + 1) + 29 * (i // 2)) % V for i in range(N)]).cuda()


def eval_fields(r):
    return dict(nll_S=r.nll_S, smooth_S=r.smooth_S, correct_S=r.correct_S, tokens_S=r.tokens_S, pred_hist_V=r.pred_hist_V, nll_BL=r.nll_BL,
                pred_BL=r.pred_BL, rank_BL=r.rank_BL, label_smooth=torch.tensor(r.label_smooth, dtype=torch.float64))    # (`loss` follows from these; reading it here would be a device-to-host transfer inside the call)


def evaluate(N, max_rows):
    def fn(vae, var):
        return eval_fields(var.evaluate(eval_tokens(N, var.L), torch.tensor(labels_of(N)), label_smooth=0.1, max_rows=max_rows))
    return fn


def distance_profile(vae, var):
    r = var.distance_profile(scoring_gt(), torch.tensor(SCORE_LABELS), [0.0, 0.5, 1.0, 2.0, 4.0, float('inf')], cfg=1.5, max_rows=5, min_prob=1e-6)
    return dict(count=r.count_NKSB, mass_q=r.mass_q_NKSB, edges=r.edges)


def class_information(prior):
    def fn(vae, var):
        r = var.class_information(scoring_gt(), torch.tensor(SCORE_LABELS), cfg=1.5, max_rows=5, prior=prior)
        return dict(entropy=r.entropy, h_mix=r.h_mix, h_cond=r.h_cond, mi=r.mi, logp_mix=r.logp_mix, prior=r.prior)
    return fn


def attention_profile(vae, var):
    r = var.attention_profile(eval_tokens(5, var.L), torch.tensor(labels_of(5)), radius=1, layers=(1,), max_rows=4, return_tokens=True)
    return dict(share_q=r.share_q, nan_queries=r.nan_queries, tokens=r.tokens)


def bad_attention_precision(vae, var):
    """refused on the host: the 16-bit workspaces hold 16-bit queries and keys (run under the f16 policy)"""
    var.attention_profile(eval_tokens(5, var.L), torch.tensor(labels_of(5)), radius=1, layers=(1,), max_rows=4, return_tokens=True)


def encode_fixture_tokens():
    z, meta = fix('encode_t_pn12345')
    return cuda_i64(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], axis=1))


def encode_fixture_image(size=None):
    """the fixture's image; size: resampled once on the host (the overlay of class_heatmaps wants size x size pixels)"""
    key = ('encode_t_pn12345 image', size)
    if key not in _FIX:
        img = torch.from_numpy(fix('encode_t_pn12345')[0]['img'])
        _FIX[key] = img if size is None else torch.nn.functional.interpolate(img, size=(size, size), mode='bilinear', align_corners=False)
    return _FIX[key].cuda()


def class_heatmaps(vae, var):
    r = var.class_heatmaps(encode_fixture_tokens(), torch.tensor(SCORE_LABELS), encode_fixture_image(64), score='log_prob', cfg=1.5, max_rows=8, size=64,
                           return_maps=True)
    return dict(lo=r.lo, hi=r.hi, pred=r.pred, margin=r.margin, area=r.area, maps=r.maps, overlays=r.overlays)


def vae_forward(image):
    def fn(vae, var):
        assert not vae.training and not torch.is_grad_enabled()
        rec, usages, loss = vae(image(), ret_usages=True)
        return dict(rec=rec, vq_loss=loss, usages=torch.tensor(usages, dtype=torch.float64))
    return fn


def vaefwd_fixture_image():
    """vaefwd_d_b3 was recorded on the deck model's tokenizer (ch 32, patch numbers 1 to 5, shared Phi 4, no znorm, the detinit weights); the other
    vaefwd_* fixtures have four scales.  Its EMA buffer is not installed (that would be state the other entries see), so `usages` is not anchored."""
    return torch.from_numpy(fix('vaefwd_d_b3')[0]['img']).cuda()


def vaefwd_anchor(res):
    from tests.test_vae_forward_gpu import LOSS_REL_BOUND, REC_ATOL           # the bounds of that file's own check against this fixture
    z, meta = fix('vaefwd_d_b3')
    t = model_meta('t')
    assert (meta['ch'], meta['patch_nums'], meta['V'], meta['share_quant_resi'], meta['using_znorm']) == (t['ch'], t['patch_nums'], t['V'], 4, False)
    ok, m = util.diff_report('VQVAE.forward rec vs reference', res['rec'].numpy(), z['rec'], atol=REC_ATOL)
    assert ok, m
    assert abs(float(res['vq_loss']) / float(z['vq_loss']) - 1) <= LOSS_REL_BOUND


def build_deck():
    deck = []

    def add(name, fn, model='t', policy='f32', autocast=False, anchor=None, raises=None):
        deck.append(Entry(name, model, policy, autocast, fn, anchor, raises))

    for prec in PRECS:                         # grouped by precision: in the listed order a mode's workspaces live through its whole group
        a = (lambda f: f) if prec == 'f32' else (lambda f: None)          # the fixtures pin the fp32 parity mode
        add(f'ar_b2[{prec}]', ar(2, 11), policy=prec)
        fn, an = e2e_fixture('t_pn12345'); add(f'e2e_t_pn12345[{prec}]', fn, policy=prec, anchor=a(an))
        add(f'ar_b5_d16[{prec}]', ar(5, 13), model='d16', policy=prec)
        add(f'ar_b3_more_smooth[{prec}]', ar(3, 12, more_smooth=True), policy=prec)
        if prec == 'f32':
            add('bad_labels', bad_labels, raises=ValueError)
        add(f'edit_a_inpaint_public[{prec}]', edit_public, policy=prec)
        add(f'edit_a_inpaint[{prec}]', edit_fixture, policy=prec, anchor=a(edit_anchor))
        fn, an = e2e_fixture('d16_pn123'); add(f'e2e_d16_pn123[{prec}]', fn, model='d16', policy=prec, anchor=a(an))
        add(f'inpainting_public[{prec}]', inpaint_public, policy=prec)
        add(f'inpaint_t_pn12345[{prec}]', inpaint_fixture, policy=prec, anchor=a(inpaint_anchor))
        for case in ('smooth_t_pn12345_count', 'smooth_t_pn12345_thr'):
            fn, an = smooth(case); add(f'{case}[{prec}]', fn, policy=prec, anchor=a(an))
        add(f'forward_eval[{prec}]', forward_eval, policy=prec, anchor=a(forward_anchor))
        if prec == 'f32':
            add('bad_gt_length', bad_gt_length, raises=ValueError)
        add(f'token_log_likelihood[{prec}]', loglik, policy=prec)
        add(f'token_scores_group_smoothed[{prec}]', scores('group_smoothed', group=50), policy=prec)
        if prec == 'f32':
            add('bad_score', bad_score, raises=ValueError)
        add(f'token_scores_neighbor_max[{prec}]', scores('neighbor_max', threshold=3.0), policy=prec)
        add(f'token_scores_expected_distance[{prec}]', scores('expected_distance', top_k=16), policy=prec)
        add(f'classify_keep[{prec}]', classify, policy=prec)
        for feat in ('vae_post', 'vae_fhat'):
            fn, an = generative(feat); add(f'classify_generative_{feat}[{prec}]', fn, policy=prec, anchor=a(an))
        # the calls merged after the first 65 entries, inside the same groups: they share the mode's workspaces with the entries above
        add(f'per_image_b3[{prec}]', per_image, policy=prec)
        add(f'evaluate[{prec}]', evaluate(5, 3), policy=prec)                  # passes of 3 + 2 rows
        add(f'ar_b2_scored[{prec}]', ar_scored, policy=prec)
        add(f'distance_profile[{prec}]', distance_profile, policy=prec)
        add(f'per_image_b2_more_smooth[{prec}]', per_image_more_smooth, policy=prec)
        add(f'class_information_uniform[{prec}]', class_information(None), policy=prec)
        if prec != 'f16':
            add(f'per_image_b5_d16[{prec}]', per_image_d16, model='d16', policy=prec)
        add(f'per_image_b3_scored[{prec}]', per_image_scored, policy=prec)
        add(f'class_information_prior[{prec}]', class_information([0.3, 0.25, 0.2, 0.1, 0.1, 0.05]), policy=prec)
        add(f'sample_best_of[{prec}]', best_of, policy=prec)
        if prec == 'f32':
            add('attention_profile[f32]', attention_profile)
        elif prec == 'f16':
            add('bad_attention_precision', bad_attention_precision, policy='f16', raises=ValueError)
        add(f'class_heatmaps[{prec}]', class_heatmaps, policy=prec)
        if prec != 'f16':
            add(f'evaluate_d16[{prec}]', evaluate(11, 8), model='d16', policy=prec)          # passes of 8 + 3 rows
        if prec == 'f32':                      # the VQVAE's own entry points run its fp32 engines whatever the VAR is set to
            add('encoder_blocks_leave_partials', encoder_blocks_leave_partials)
            add('vae_img_to_idxBl', vae_encode, anchor=vae_encode_anchor)
            add('vae_fhat_to_img', vae_decode_fhat)
            add('vae_idxBl_to_img', vae_decode_tokens)
            add('vae_forward', vae_forward(encode_fixture_image))
            add('vae_forward_d_b3', vae_forward(vaefwd_fixture_image), anchor=vaefwd_anchor)
    add('ar_b2[auto under fp16 autocast]', ar(2, 11), policy='auto', autocast=True)
    assert len({e.name for e in deck}) == len(deck)
    assert len(deck) == 65 + 38 and sum(e.raises is not None for e in deck) == 4 and sum(e.model == 'd16' for e in deck) == 6 + 4
    return deck


DECK = build_deck()
BY_NAME = {e.name: e for e in DECK}


# ---- running and comparing ---------------------------------------------------------------------------------------------------------------
def run(e, vae, var):
    """one deck entry on the given model -> its full result on the host"""
    var.set_hip_precision(e.policy)
    ctx = torch.autocast('cuda', dtype=torch.float16) if e.autocast else contextlib.nullcontext()
    with torch.no_grad(), ctx:                 # (not inference_mode: tensors made there carry no version counter and the engines' caches would not be exercised)
        if e.raises is not None:
            with pytest.raises(e.raises):
                e.fn(vae, var)
            return {'raised': e.raises.__name__}
        out = e.fn(vae, var)
        torch.cuda.synchronize()
        return {k: v.detach().cpu() for k, v in out.items()}


def alone(e):
    if e.name not in _ALONE:
        vae, var = fresh(e.model)
        _ALONE[e.name] = run(e, vae, var)
        del vae, var
    return _ALONE[e.name]


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def difference(got, want):
    """None when the two results are the same bits (NaN patterns and signed zeros included), else what differs first"""
    if got.keys() != want.keys():
        return f'keys {sorted(got)} != {sorted(want)}'
    for k in want:
        g, w = got[k], want[k]
        if not torch.is_tensor(w):
            if g != w: return f'{k}: {g!r} != {w!r}'
        elif g.dtype != w.dtype or g.shape != w.shape:
            return f'{k}: {g.dtype} {tuple(g.shape)} != {w.dtype} {tuple(w.shape)}'
        elif not torch.equal(bits(g), bits(w)):
            ne = (g != w) & ~(torch.isnan(g) & torch.isnan(w)) if g.is_floating_point() else (g != w)
            return f'{k}: {int(ne.sum())} of {g.numel()} elements differ, {int(torch.isnan(g).sum()) if g.is_floating_point() else 0} NaN in the result'
    return None


def order_of(which):
    if which == 'listed':
        order = list(DECK)
    elif which == 'reverse':
        order = list(reversed(DECK))
    else:
        order = [DECK[i] for i in np.random.default_rng(int(which[len('perm'):])).permutation(len(DECK))]
    while order[-1].raises is not None:        # a refused call is always followed by a normal one
        order.insert(0, order.pop())
    return order


def run_order(which, before_each=None):
    bad, prev = [], '(nothing: the first call of this pass)'
    for e in order_of(which):
        vae, var = company(e.model)
        want = alone(e)
        if before_each is not None:
            before_each()
        d = difference(run(e, vae, var), want)
        if d is not None:
            bad.append(f'{e.name}, order {which}, right after {prev}: {d}')
        prev = e.name
    assert not bad, f'{len(bad)} of {len(DECK)} calls differ from the same call made first on a fresh model:\n' + '\n'.join(bad)


# ---- alone / in company ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('group', PRECS)
def test_alone_every_entry_runs_first_on_its_own_fresh_model(group):
    """the alone results, one fresh model each, computed a precision group at a time (the 'auto' entry with f16) so that no single test carries
    all of the builds; every later test takes them from the cache"""
    mine = [e for e in DECK if (e.policy if e.policy != 'auto' else 'f16') == group]
    assert mine and sum(len([e for e in DECK if (e.policy if e.policy != 'auto' else 'f16') == g]) for g in PRECS) == len(DECK)
    for e in mine:
        res = alone(e)
        assert res and (e.raises is None) == ('raised' not in res), e.name


def test_alone_results_are_anchored_to_the_reference_fixtures():
    bad = []
    for e in DECK:
        res = alone(e)
        if e.anchor is not None:
            try:
                e.anchor(res)
            except AssertionError as err:
                bad.append(f'{e.name}: {err}')
    assert not bad, '\n'.join(bad)
    # 'auto' inside an fp16 autocast region is the explicit f16 mode
    assert difference(alone(BY_NAME['ar_b2[auto under fp16 autocast]']), alone(BY_NAME['ar_b2[f16]'])) is None
    assert difference(alone(BY_NAME['ar_b2[f16]']), alone(BY_NAME['ar_b2[f32]'])) is not None, 'the 16-bit mode did not run'
    # the partials route and the statistics pass of GroupNorm give the same bits
    r = alone(BY_NAME['encoder_blocks_leave_partials'])
    assert torch.equal(r['gn_own_full'], r['gn_own_part'])
    assert torch.equal(r['gn_other'], r['gn_other_want']), 'gn() used the partials a conv left for another tensor'
    # the scored calls promise the images and tokens of the calls they extend, bit for bit
    for prec in PRECS:
        scored, plain = alone(BY_NAME[f'ar_b2_scored[{prec}]']), alone(BY_NAME[f'ar_b2[{prec}]'])
        assert difference(dict(img=scored['images']), plain) is None, f'autoregressive_infer_cfg_scored[{prec}]: images differ from autoregressive_infer_cfg'
        scored, plain = alone(BY_NAME[f'per_image_b3_scored[{prec}]']), alone(BY_NAME[f'per_image_b3[{prec}]'])
        assert difference(dict(tokens=scored['tokens']), dict(tokens=plain['tokens'])) is None, f'per_image_scored[{prec}]: tokens differ from the per-image call'


@pytest.mark.parametrize('which', ['listed', 'reverse', 'perm0', 'perm1', 'perm2'])
def test_in_company_every_call_equals_its_alone_result(which):
    run_order(which)


# ---- poisoned ----------------------------------------------------------------------------------------------------------------------------
def tensors_in(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values(): yield from tensors_in(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj: yield from tensors_in(v)


# Every attribute of an engine under which a tensor outlives a call is on one of these two lists (the state table); an attribute
# on neither fails test_every_tensor_an_engine_keeps_is_poisoned_or_derived_from_the_weights with its name.
POISONED = {                                   # overwritten before every call of the poisoned pass
    'SamplingEngine._ws', 'SamplingEngine._ws_tf',                      # the buffer sets (`class_mix`, `masked`, `probs`, `h` and the views in `ada_view` hang in them)
    'SamplingEngine.last_trace', 'SamplingEngine.last_smooth',          # outputs of the last call: nothing may read them back
    'DecoderEngine._gn_part', 'EncoderEngine._gn_part',                 # pending GroupNorm partials
}
DERIVED = {                                    # copies and tables made from the weights, keyed on the weight signature; the checked label tensor
    'SamplingEngine.w', 'SamplingEngine._labels_ok',
    'DecoderEngine.w', 'DecoderEngine.w16s', 'EncoderEngine.w', 'EncoderEngine.w16s',
    'QuantizerEngine.codebook', 'QuantizerEngine.phi', 'QuantizerEngine._taps',
}


def engines_of(vae, var):
    """the live engine objects of a model pair: the sampling engine with its decoder, encoder and quantizer engines, and the VQVAE's own two"""
    eng = var.engine()
    found = [eng, eng.dec, vae._hip_decoder, vae._hip_encoder, getattr(var.vae_quant_proxy[0], '_hip_engine', None), getattr(vae.quantize, '_hip_engine', None)]
    out = []
    for e in found:
        if e is not None and not any(e is o for o in out):
            out.append(e)
    return out


def kept_tensors(vae, var):
    """{'<engine class>.<attribute>': [tensors]}: every tensor reachable from an engine's own attributes through dicts, lists and tuples"""
    found = {}
    for e in engines_of(vae, var):
        for attr, val in vars(e).items():
            ts = list(tensors_in(val))
            if ts:
                found.setdefault(f'{type(e).__name__}.{attr}', []).extend(ts)
    return found


def poison_engines(vae, var):
    """every tensor the engines keep between calls gets the guard bands' byte (tests/util.py): 0xFF — NaN in fp32 / fp16 / bf16 / fp64, 255 in a
    uint8 map; integer buffers get V - 1, a legal index, so that a stale read changes the result and not the address it reads from.
    -> the number of tensors written"""
    roots = [ts for name, ts in kept_tensors(vae, var).items() if name in POISONED]
    n = 0
    for t in tensors_in(roots):
        if t.numel() == 0:
            continue
        if t.is_floating_point():
            if t.is_contiguous(): bits(t).fill_(0xFF)
            else: t.fill_(float('nan'))           # (a strided view of a buffer that is in the workspace itself)
        elif t.dtype in (torch.uint8, torch.bool):
            t.fill_(255 if t.dtype == torch.uint8 else True)
        else:
            t.fill_(var.V - 1)
        n += 1
    return n


def poison_allocator():
    """best effort, not an assertion: NaN-filled blocks of a call's sizes are handed back to the caching allocator, so that the torch.empty
    temporaries of the next call likely come out of poisoned memory"""
    sizes = [32 << 20, 8 << 20] + [1 << 20] * 4 + [256 << 10] * 8 + [64 << 10] * 16 + [4 << 10] * 16
    blocks = [torch.full((s // 4,), float('nan'), device='cuda') for s in sizes]
    del blocks


def test_poisoned_workspaces_change_nothing():
    """nothing is read before the current call wrote it: the KV caches past the current position, up, pooled, f_hat, idx, hid, the
    teacher-forcing workspaces, pending GroupNorm partials"""
    for kind in ('t', 'd16'):
        if kind not in _COMPANY:               # (run on its own: give the models a history first)
            run_order('listed')
            break
    written = []

    def before_each():
        torch.cuda.synchronize()
        written.append(sum(poison_engines(*_COMPANY[k]) for k in _COMPANY))
        poison_allocator()
        torch.cuda.synchronize()
    run_order('perm0', before_each)
    print(f'poisoned pass: {len(written)} calls, {min(written)} to {max(written)} engine tensors overwritten before each')
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'


def unlisted_kept_tensors(vae, var):
    found = kept_tensors(vae, var)
    return sorted(f'{name} ({len(ts)} tensors)' for name, ts in found.items() if name not in POISONED and name not in DERIVED), found


def test_every_tensor_an_engine_keeps_is_poisoned_or_derived_from_the_weights():
    """the poisoned pass is complete: after the whole deck ran, every tensor that hangs on an engine is either overwritten by poison_engines or a
    copy of the weights under the weight signature.  A call that parks a buffer anywhere else fails here, with the attribute's name."""
    if set(_COMPANY) != {'t', 'd16'}:          # (run on its own: the full listed pass first)
        run_order('listed')
    for kind in ('t', 'd16'):
        vae, var = _COMPANY[kind]
        names = sorted(type(e).__name__ for e in engines_of(vae, var))
        assert names == (['DecoderEngine', 'EncoderEngine', 'QuantizerEngine', 'SamplingEngine'] if kind == 't' else ['DecoderEngine', 'QuantizerEngine', 'SamplingEngine']), names
        unlisted, found = unlisted_kept_tensors(vae, var)
        print(f'{kind}: ' + ', '.join(f'{name}: {len(ts)}' for name, ts in sorted(found.items())))
        assert not unlisted, f'{kind}: tensors outlive a call under attributes that are neither poisoned nor listed as derived from the weights: {unlisted}'
        # (which buffer sets are alive depends on the last call: a precision switch drops the other modes'; the weight copies always are)
        want = {'SamplingEngine.w', 'DecoderEngine.w', 'QuantizerEngine.codebook'} | ({'EncoderEngine.w'} if kind == 't' else set())
        assert want <= set(found), f'{kind}: the walk misses {sorted(want - set(found))}'
    # the walk sees a buffer parked on an engine: a tensor hung on an unlisted attribute is reported by name, and found again inside a container
    eng = _COMPANY['t'][1].engine()
    eng.parked_by_the_test = {'a': [torch.zeros(3, device='cuda')]}
    try:
        assert unlisted_kept_tensors(*_COMPANY['t'])[0] == ['SamplingEngine.parked_by_the_test (1 tensors)']
    finally:
        del eng.parked_by_the_test


# ---- workspaces --------------------------------------------------------------------------------------------------------------------------
def ar_entry(B, seed, policy='f32'):
    return Entry(f'ar_b{B}_seed{seed}[{policy}]', 't', policy, False, ar(B, seed), None, None)


def test_workspaces_across_batch_sizes_streams_and_precisions():
    vae, var = fresh('t')
    eng = var.engine()
    bad = []

    def check(e, got, where):
        d = difference(got, alone(e))
        if d is not None: bad.append(f'{e.name} {where}: {d}')

    # eight batch sizes on one stream, largest first and mixed: a smaller call runs over the rows a larger one left
    for B in (8, 1, 5, 2, 7, 3, 6, 4):
        e = ar_entry(B, 20 + B)
        check(e, run(e, vae, var), 'after other batch sizes on one stream')
        assert len(eng._ws) <= eng.MAX_WORKSPACES
    # two batch sizes alternately on two side streams, both calls in flight (tests/test_e2e_gpu.py::test_calls_in_flight_on_two_streams)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    plan = [((3, 6)[(i // 2) % 2], 40 + i % 2, i % 2) for i in range(8)]
    outs = []
    var.set_hip_precision('f32')
    with torch.no_grad():
        for B, seed, s in plan:
            with torch.cuda.stream(streams[s]):
                outs.append(ar(B, seed)(vae, var)['img'])
    torch.cuda.synchronize()
    for (B, seed, s), img in zip(plan, outs):
        check(ar_entry(B, seed), dict(img=img.cpu()), f'in flight on stream {s}')
    assert len(eng._ws) <= eng.MAX_WORKSPACES
    slots = collections.Counter(k[1:] for k in eng._ws)
    assert max(slots.values()) == 1, f'more than one buffer set per (stream, precision): {dict(slots)}'
    assert len({k[1] for k in eng._ws}) >= 2, 'the two streams shared a workspace'
    # a precision switch between two calls of the same batch size, and back
    for policy in ('f32', 'f16', 'f32', 'bf16', 'f32'):
        e = ar_entry(4, 24, policy)
        check(e, run(e, vae, var), 'after a precision switch')
    assert len(eng._ws) <= eng.MAX_WORKSPACES and len(eng._ws_tf) <= eng.MAX_WORKSPACES
    assert not bad, '\n'.join(bad)


def tf_entry(name, fn, policy='f32'):
    return Entry(f'{name}[{policy}]', 't', policy, False, fn, None, None)


def loglik_rows(K, cfg, max_rows):
    def fn(vae, var):
        return dict(lp=var.token_log_likelihood(scoring_gt(), torch.tensor(SCORE_LABELS[:K]), cfg=cfg, max_rows=max_rows))
    return fn


def classify_rows(K, keep):
    def fn(vae, var):
        r = var.classify(scoring_gt(), torch.tensor(SCORE_LABELS[:K]), 'log_prob', cfg=1.5, max_rows=8, keep=keep)
        return dict(pred=r.pred, total=r.total, depth=r.depth, tokens=r.tokens)
    return fn


def test_teacher_forced_workspaces_across_rows_streams_and_precisions():
    """the teacher-forced family shares SamplingEngine._tf_workspace: KV caches allocated once and never cleared, one row count resident per
    (stream, precision, L_e), a pass of fewer rows on a prefix.  Row counts R = images_in_pass x (classes_in_pass + [cfg > 0]) for the scoring
    calls, min(max_rows, N) for evaluate."""
    vae, var = fresh('t')
    eng = var.engine()
    L = var.L
    bad = []

    def check(e, got, where):
        d = difference(got, alone(e))
        if d is not None: bad.append(f'{e.name} {where}: {d}')

    def rows_resident(Le=None):
        sid = int(torch.cuda.current_stream().cuda_stream)
        return sorted(k[0] for k in eng._ws_tf if k[1:] == (sid, 'f32', L if Le is None else Le))

    # row counts on one stream, the largest first, then alternately below and above the one before; classify(keep=...) in between creates the
    # shorter L_e sets (L_e = 5 and 14 beside 55), the second time at other row counts, which evicts the first ones
    plan = [(8, tf_entry('loglik_K3_cfg_rows8', loglik_rows(3, 1.5, 8))),          # 2 images x (3 + 1)
            (1, tf_entry('evaluate_N5_rows1', evaluate(5, 1))),
            (6, tf_entry('loglik_K2_cfg_rows6', loglik_rows(2, 1.5, 6))),          # 2 x (2 + 1)
            (None, tf_entry('classify_K6_keep32', classify_rows(6, {1: 3, 2: 2}))),      # L_e = 5: 2 x (6 + 1) rows, L_e = 14: 2 x (3 + 1)
            (2, tf_entry('evaluate_N5_rows2', evaluate(5, 2))),                     # 2 + 2 + 1
            (7, tf_entry('loglik_K6_cfg_rows7', loglik_rows(6, 1.5, 7))),          # 1 x (6 + 1)
            (3, tf_entry('evaluate_N5_rows3', evaluate(5, 3))),                     # 3 + 2
            (None, tf_entry('classify_K5_keep42', classify_rows(5, {1: 4, 2: 2}))),      # L_e = 5: 2 x (5 + 1) rows, L_e = 14: 2 x (4 + 1)
            (5, tf_entry('loglik_K6_cfg_rows5', loglik_rows(6, 1.5, 5))),          # 1 x (4 + 1), then 1 x (2 + 1) on a prefix
            (1, tf_entry('loglik_K1_rows1', loglik_rows(1, 0.0, 1))),
            (4, tf_entry('evaluate_N5_rows4', evaluate(5, 4)))]                     # 4 + 1
    seen, short = [], set()
    for R, e in plan:
        check(e, run(e, vae, var), f'after the row counts {seen} on one stream')
        if R is not None:
            assert rows_resident() == [R], f'{e.name}: expected one set of {R} rows at L_e = {L}, found {rows_resident()}'
            seen.append(R)
        else:
            short |= {(k[0], k[3]) for k in eng._ws_tf if k[3] < L}
        assert len(eng._ws_tf) <= eng.MAX_WORKSPACES
    assert len(set(seen)) >= 6 and 1 in seen and all((b - a) * (c - b) < 0 for a, b, c in zip(seen, seen[1:], seen[2:])), seen
    assert len({Le for _, Le in short}) >= 2 and len(short) > len({Le for _, Le in short}), f'classify did not create and replace the shorter sets: {sorted(short)}'

    # two side streams: A runs the scoring calls and the after_block hook, B samples and evaluates.  The test adds no synchronisation between the
    # calls and reads no result before the final synchronize(); what a call does itself stays: its label / token range check reads two numbers
    # back, which drains the issuing stream only, so each stream's kernels run while the host issues the other stream's next call
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    names = (['token_log_likelihood[f32]', 'class_information_uniform[f32]', 'attention_profile[f32]'],
             ['ar_b2[f32]', 'per_image_b3[f32]', 'evaluate[f32]'])
    outs = []
    var.set_hip_precision('f32')
    with torch.no_grad():
        for i in range(6):
            for s in (0, 1):
                e = BY_NAME[names[s][i % 3]]
                with torch.cuda.stream(streams[s]):
                    outs.append((e, s, e.fn(vae, var)))
    torch.cuda.synchronize()
    for e, s, out in outs:
        check(e, {k: v.detach().cpu() for k, v in out.items()}, f'in flight on stream {s}')
    slots = collections.Counter(k[1:] for k in eng._ws_tf)
    assert max(slots.values()) == 1, f'more than one buffer set per (stream, precision, L_e): {dict(slots)}'
    assert len({k[1] for k in eng._ws_tf}) >= 2, 'the two streams shared a teacher-forcing workspace'
    assert len(eng._ws) <= eng.MAX_WORKSPACES and len(eng._ws_tf) <= eng.MAX_WORKSPACES

    # precision switches between identical calls, and back
    for policy in ('f32', 'bf16', 'f32'):
        for name in ('evaluate', 'distance_profile'):
            e = BY_NAME[f'{name}[{policy}]']
            check(e, run(e, vae, var), 'after a precision switch')
    assert len(eng._ws) <= eng.MAX_WORKSPACES and len(eng._ws_tf) <= eng.MAX_WORKSPACES
    assert not bad, '\n'.join(bad)


# ---- derived weight copies at recycled addresses -------------------------------------------------------------------------------------------
def replace_parameter(module, name, values_host):
    """drop module.<name>, release it, install a new nn.Parameter of the same shape holding values_host, with the old version counter
    -> (the new parameter landed on the old address, with an equal version counter)"""
    old = getattr(module, name)
    addr, ver, shape, dev = old.data_ptr(), old._version, tuple(old.shape), old.device
    setattr(module, name, None)                # (the slot stays, so module.parameters() keeps its order: only the tensor changes)
    del old
    gc.collect()
    torch.cuda.synchronize()
    missed = []
    # the freed block is handed out after every free block of its size at a lower address: a 512-byte q_bias waits behind whatever small tensors
    # the calls before it released, so the search is bounded by bytes (64 MiB of misses), not by a fixed sixteen tries
    nbytes = 4 * max(1, int(np.prod(shape)))
    for attempt in range(max(16, min(4096, (64 << 20) // nbytes))):
        p = torch.nn.Parameter(torch.empty(shape, dtype=torch.float32, device=dev), requires_grad=False)
        if p.data_ptr() == addr:
            break
        missed.append(p)                       # keep the miss allocated: the next request gets another block
    p.data.copy_(values_host)                  # (through .data: no counter moves)
    with torch.no_grad():
        while p._version < ver:
            p.add_(0)
    del missed
    setattr(module, name, p)
    return p.data_ptr() == addr and p._version == ver, (addr, ver, p.data_ptr(), p._version, attempt + 1)


PARAMETERS = dict(ada_lin=lambda vae, var: (var.blocks[0].ada_lin[1], 'weight'), q_bias=lambda vae, var: (var.blocks[1].attn, 'q_bias'),
                  phi=lambda vae, var: (list(vae.quantize.quant_resi.phis())[0], 'weight'), decoder_conv=lambda vae, var: (vae.decoder.conv_in, 'weight'),
                  codebook=lambda vae, var: (vae.quantize.embedding, 'weight'), head=lambda vae, var: (var.head, 'weight'),
                  word_embed=lambda vae, var: (var.word_embed, 'weight'))
# of these the engines keep the parameter's own storage (a detached alias in `w` / QuantizerEngine.codebook) beside the tables derived from it:
# while the old copies live the address cannot come back, so there is no collision to wait for; the stale-copy assertion holds all the same
STORAGE_HELD = ('codebook', 'head', 'word_embed')


@pytest.mark.parametrize('which,entry', [
    pytest.param('ada_lin', 'ar_b2[f32]', id='ada_lin'), pytest.param('q_bias', 'ar_b2[f32]', id='q_bias'),
    pytest.param('phi', 'ar_b2[f32]', id='phi'), pytest.param('decoder_conv', 'ar_b2[f32]', id='decoder_conv'),
    pytest.param('codebook', 'token_scores_neighbor_max[f32]', id='codebook-neighbor_max'),                # code_dist, thresholded
    pytest.param('codebook', 'smooth_t_pn12345_count[f32]', id='codebook-smooth_sampling'),                # w['nbr']: neighbor_table's only reader
    pytest.param('codebook', 'token_scores_expected_distance[f32]', id='codebook-expected_distance'),      # code_dist
    pytest.param('codebook', 'distance_profile[f32]', id='codebook-distance_profile'),                     # code_dist
    pytest.param('codebook', 'ar_b3_more_smooth[f32]', id='codebook-more_smooth'),                         # codebook_T
    pytest.param('head', 'evaluate[bf16]', id='head-evaluate_bf16'),                                       # head_w16
    pytest.param('word_embed', 'token_log_likelihood[f32]', id='word_embed-token_log_likelihood'),         # the teacher-forced pass
])
def test_replaced_parameter_at_a_recycled_address(which, entry):
    """ada_lin, q_bias, phi, decoder_conv: the engines hold only a packed copy of these parameters (ada_w_all, qkv_b, the channels-last Phi kernel,
    the re-laid decoder kernel), so nothing of theirs keeps the parameter's storage: a replacement lands on the old address with the old
    version counter.  codebook, head, word_embed: the engine holds the storage itself and tables DERIVED from it (code_dist, nbr, codebook_T,
    head_w16), built by the first call below.  Without invalidate_engine() the next call must compute with the new values either way: equal
    to a fresh model carrying them."""
    pick = PARAMETERS[which]
    e = BY_NAME[entry]

    def holders(vae, var):
        """the engine attributes that hold the parameter's own storage (a tensor at its address), after the first call"""
        m, n = pick(vae, var)
        addr = getattr(m, n).data_ptr()
        return sorted(name for name, ts in kept_tensors(vae, var).items() if any(t.data_ptr() == addr for t in ts))

    def new_values(vae, var):
        m, n = pick(vae, var)
        p = getattr(m, n).detach().cpu()
        return p.flip(0) * 0.75 + 0.01

    vae, var = fresh('t')
    base = run(e, vae, var)
    held = holders(vae, var)
    assert bool(held) == (which in STORAGE_HELD), f'{which}: the engines hold its storage under {held}; STORAGE_HELD says {which in STORAGE_HELD}'
    vals = new_values(vae, var)
    hit, info = replace_parameter(*pick(vae, var), vals)
    print(f'{which}: old (address, version) = ({info[0]:#x}, {info[1]}), new = ({info[2]:#x}, {info[3]}): '
          f"{'RECYCLED address with an equal version counter' if hit else 'no collision'} after {info[4]} tries")
    got = run(e, vae, var)                      # no invalidate_engine()
    del vae, var
    vae2, var2 = fresh('t')
    m2, n2 = pick(vae2, var2)
    with torch.no_grad():
        getattr(m2, n2).copy_(vals)             # (before the first call: nothing is packed yet)
    want = run(e, vae2, var2)
    assert difference(want, base) is not None, 'the new values do not change the result: the test would prove nothing'
    d = difference(got, want)
    assert d is None, f'{which}: the engine computed with a stale packed copy ({"address recycled" if hit else "no collision"}): {d}'
    if held:
        print(f'{which}: the engine keeps this parameter\'s own storage alive ({", ".join(held)}) beside the derived tables, so its address cannot be recycled '
              f'({"it was all the same" if hit else "it was not"}): the precondition does not apply')
        return
    assert hit, (f'{which}: precondition not met — in {info[4]} tries the allocator did not hand the freed block back with an equal version counter '
                 f'(old {info[0]:#x} v{info[1]}, new {info[2]:#x} v{info[3]}), so the recycled-address case was not exercised')


# ---- the label check ---------------------------------------------------------------------------------------------------------------------
def test_label_check_refuses_a_bad_label_at_a_recycled_address():
    """the caller's usual pattern, label_B=torch.tensor([...], device='cuda') per call: the caching allocator hands the freed block to the next
    request of the same size, so the second tensor has the first one's address, length and version 0.  Only _check_labels is called: no
    kernel ever sees the label."""
    vae, var = fresh('t')
    eng = var.engine()
    assert var.num_classes == 1000
    reused = 0
    for trial in range(8):
        a = torch.tensor([1, 2, 3, 4], device='cuda')
        eng._check_labels(a)
        ident = (a.data_ptr(), a._version, a.numel(), a.device)
        del a
        b = torch.tensor([5000, 2, 3, 4], device='cuda')
        same = (b.data_ptr(), b._version, b.numel(), b.device) == ident
        reused += int(same)
        print(f'trial {trial}: checked {ident[0]:#x} v{ident[1]}, next tensor at {b.data_ptr():#x} v{b._version}: address {"REUSED" if same else "not reused"}')
        with pytest.raises(ValueError, match='labels must lie in'):
            eng._check_labels(b)
        del b
    print(f'the address was reused in {reused} of 8 trials')
    # and the saving stands: the same tensor, unwritten, is checked once
    c = torch.tensor([0, 999, 1000, 5], device='cuda')
    real, calls = torch.aminmax, []
    torch.aminmax = lambda *a_, **k: calls.append(1) or real(*a_, **k)
    try:
        eng._check_labels(c); eng._check_labels(c)
    finally:
        torch.aminmax = real
    assert len(calls) == 1
