"""History independence of the engines on a real MI355X: the result of a public call depends on the weights, the arguments,
the seed and the precision, never on what the model object did before.

A fixed deck of calls (sampling at several batch sizes, editing, inpainting, smooth sampling, the teacher-forced forward, the scoring and
classification calls, the VQVAE's own entry points, three calls that are refused on the host; every call that has 16-bit modes in f32, f16 and
bf16, one under 'auto' inside an autocast region) is run
  alone        each entry as the FIRST call on a model nothing has touched; where a fixture under tests/golden pins the call, its tokens are
               asserted against the reference's, so "alone" is anchored to the reference and not only to itself;
  in company   on ONE model per configuration that is never rebuilt: the deck in its listed order, reversed, and in three seeded permutations;
  poisoned     one more pass, with every workspace tensor the engines keep between calls overwritten before each call (0xFF bytes: NaN in every
               float format, 255 in uint8 maps; V - 1, a legal index, in integer buffers) and a NaN-filled block handed back to the allocator.
Every result must equal the entry's alone result BIT FOR BIT (the fp32 path is under a bit-exactness contract, the 16-bit kernels are asserted
run-to-run deterministic, 'auto' is asserted bit-equal to the explicit modes: no tolerance is needed or used).

Then: workspaces across eight batch sizes, two streams in flight and a precision switch; a parameter replaced by a new one that lands on the
old one's address with the old one's version counter; the label range check against a recycled address (through _check_labels alone: no kernel
ever sees the bad label).  Every call in this file is a legal call."""
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
        if prec == 'f32':                      # the VQVAE's own entry points run its fp32 engines whatever the VAR is set to
            add('encoder_blocks_leave_partials', encoder_blocks_leave_partials)
            add('vae_img_to_idxBl', vae_encode, anchor=vae_encode_anchor)
            add('vae_fhat_to_img', vae_decode_fhat)
            add('vae_idxBl_to_img', vae_decode_tokens)
    add('ar_b2[auto under fp16 autocast]', ar(2, 11), policy='auto', autocast=True)
    assert len({e.name for e in deck}) == len(deck)
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


def poison_engines(vae, var):
    """every tensor the engines keep between calls gets the guard bands' byte (tests/util.py): 0xFF — NaN in fp32 / fp16 / bf16 / fp64, 255 in a
    uint8 map; integer buffers get V - 1, a legal index, so that a stale read changes the result and not the address it reads from.
    -> the number of tensors written"""
    eng = var.engine()
    roots = [eng._ws, eng._ws_tf]
    for e in (vae._hip_decoder, vae._hip_encoder):
        if e is not None and e._gn_part is not None:
            roots.append([t for t in e._gn_part if torch.is_tensor(t)])
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
    for attempt in range(16):
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
    return p.data_ptr() == addr and p._version == ver, (addr, ver, p.data_ptr(), p._version)


@pytest.mark.parametrize('which', ['ada_lin', 'q_bias', 'phi', 'decoder_conv'])
def test_replaced_parameter_at_a_recycled_address(which):
    """the engines hold only a packed copy of these parameters (ada_w_all, qkv_b, the channels-last Phi kernel, the re-laid decoder kernel), so
    nothing of theirs keeps the parameter's storage: a replacement lands on the old address with the old version counter.  Without
    invalidate_engine() the next call must still compute with the new values: equal to a fresh model carrying them."""
    pick = dict(ada_lin=lambda vae, var: (var.blocks[0].ada_lin[1], 'weight'), q_bias=lambda vae, var: (var.blocks[1].attn, 'q_bias'),
                phi=lambda vae, var: (list(vae.quantize.quant_resi.phis())[0], 'weight'), decoder_conv=lambda vae, var: (vae.decoder.conv_in, 'weight'))[which]
    e = BY_NAME['ar_b2[f32]']

    def new_values(vae, var):
        m, n = pick(vae, var)
        p = getattr(m, n).detach().cpu()
        return p.flip(0) * 0.75 + 0.01

    vae, var = fresh('t')
    base = run(e, vae, var)
    vals = new_values(vae, var)
    hit, info = replace_parameter(*pick(vae, var), vals)
    print(f'{which}: old (address, version) = ({info[0]:#x}, {info[1]}), new = ({info[2]:#x}, {info[3]}): '
          f"{'RECYCLED address with an equal version counter' if hit else 'no collision'}")
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
    assert hit, (f'{which}: precondition not met — in 16 tries the allocator did not hand the freed block back with an equal version counter '
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
