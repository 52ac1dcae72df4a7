"""VAR.sample_controlled on the MI355X: default controls against the per-image scored call in the three precisions, the logit
lens, logp_drawn against float64, batch invariance under mixed controls and schedules, a per-scale schedule rebuilt from kernel-level calls,
the ban and greedy identities, and the PyTorch twin."""
import contextlib
import io

import numpy as np
import pytest

from tests import ctlref, util
from tests import samplestatsref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

PNS, DEPTH, CH = (1, 2, 3, 4, 5), 2, 32
S = len(PNS)
_MODELS = {}
FIELDS = ('tokens', 'logp_cond', 'logp_guided', 'logp_drawn', 'entropy', 'kept')
DECK = dict(labels=[3, 980, 22, 1000], seeds=[17, 3, (1 << 62) + 5, 0], cfg=[4.0, 1.5, 0.0, 2.5], top_k=[0, 900, 1, 600], top_p=[0.96, 0.0, 0.0, 0.5])


def _model(pns=PNS, device='cuda'):
    key = (pns, device)
    if key not in _MODELS:
        from models import build_vae_var
        from var_amd.detinit import fill_module_, fill_module_device_
        fill = fill_module_device_ if device == 'cuda' else fill_module_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device=device, patch_nums=pns, depth=DEPTH, ch=CH)
        fill(var, DEPTH, 0, 'var.'); fill(vae, DEPTH, 0, 'vae.')
        _MODELS[key] = (vae.eval(), var.eval())
    return _MODELS[key]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what='', fields=FIELDS):
    for k in fields:
        assert torch.equal(_bits(getattr(a, k)), _bits(getattr(b, k))), f'{what}{k} differs'


def _bias(V, seed, bans=True):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal(V).astype(np.float32)
    if bans:
        b[rng.permutation(V)[:V // 3]] = -np.inf
    return b


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16'])
def test_default_controls_are_the_per_image_scored_call(prec):
    vae, var = _model()
    var.set_hip_precision(prec)
    try:
        d = DECK
        kw = dict(cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'])
        ref = var.autoregressive_infer_cfg_per_image_scored(d['labels'], d['seeds'], **kw)
        ref_img = ref.images.clone()
        got = var.sample_controlled(d['labels'], d['seeds'], **kw)
        _same(got, ref, prec + ': ')
        assert torch.equal(_bits(got.images), _bits(ref_img)), f'{prec}: images differ'
        assert got.tokens.shape == (4, var.L) and got.patch_nums == PNS and int(got.tokens.min()) >= 0
        nod = var.sample_controlled(d['labels'], d['seeds'], decode=False, temperature=np.ones((S, 1)), min_p=[0.0] * 4, **kw)
        assert nod.images is None
        _same(nod, ref, prec + ' explicit neutral controls: ')
    finally:
        var.set_hip_precision('f32')


def test_logp_guided_is_token_log_likelihood_under_active_controls():
    vae, var = _model()
    d = DECK
    r = var.sample_controlled(d['labels'], d['seeds'], cfg=1.5, top_k=[0, 900, 0, 600], top_p=[0.0, 0.9, 0.0, 0.5], temperature=[0.6, 1.4, 1.0, 0.9],
                              min_p=[0.05, 0.0, 0.3, 0.01], logit_bias=np.stack([_bias(var.V, i) for i in range(4)]), decode=False)
    assert int(r.tokens.min()) >= 0
    lab = torch.tensor(d['labels']).view(-1, 1)
    assert torch.equal(_bits(var.token_log_likelihood(r.tokens, lab, cfg=1.5)[:, 0]), _bits(r.logp_guided))
    assert torch.equal(_bits(var.token_log_likelihood(r.tokens, lab, cfg=0.0)[:, 0]), _bits(r.logp_cond))
    plain = var.sample_controlled(d['labels'], d['seeds'], cfg=1.5, decode=False)
    assert not torch.equal(plain.tokens, r.tokens) and bool((r.kept < plain.kept).all())


def _traced(var, labels, seeds, **kw):
    """the engine's controlled call with its trace: (tokens, stats, per-scale logits [2B, l, V], the tables)"""
    from var_amd.engine import control_tables
    B = len(seeds)
    a = dict(cfg=1.5, top_k=0, top_p=0.0, temperature=1.0, min_p=0.0, logit_bias=None, cfg_ramp=True)
    a.update(kw)
    tab = control_tables(a['cfg'], a['top_k'], a['top_p'], a['temperature'], a['min_p'], a['logit_bias'], S, var.V, B, a['cfg_ramp'])
    tok = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
    st = {}
    eng = var.engine()
    eng.sample_controlled(torch.tensor(labels, device='cuda'), seeds, tab, tokens_out=tok, decode=False, stats=st, trace=True)
    return tok, st, [z.clone() for z in eng.last_trace['logits']], tab


def test_logp_drawn_is_the_float64_log_softmax_of_the_tempered_row():
    """no filters, temperature tau: the row the token was drawn from is the fp32 row x / tau (one fp32 division per element, formed here in
    numpy as the kernel forms it); its log_softmax is evaluated in float64 and the kernel's fp32 value must lie within
    tests/samplestatsref.py's lp_bound, the bar derived there for lp_drawn on an fp32 row"""
    vae, var = _model()
    d = DECK
    taus = [0.5, 1.7, 1.0, 0.8]
    tok, st, logits, tab = _traced(var, d['labels'], d['seeds'], cfg=d['cfg'], temperature=taus)
    r = var.sample_controlled(d['labels'], d['seeds'], cfg=d['cfg'], temperature=taus, decode=False)
    assert torch.equal(r.tokens, tok) and torch.equal(_bits(r.logp_drawn), _bits(st['logp_drawn']))
    B, V, worst = 4, var.V, 0.0
    for si, (b0, e0) in enumerate(var.begin_ends):
        l = e0 - b0
        x = R.guided_rows(logits[si].cpu().numpy(), B, l, tab['t'][si]).reshape(B, l, V)
        z = np.stack([ctlref.bias_temper(x[b], None, taus[b]) for b in range(B)]).reshape(B * l, V)
        want = R._logp_rows(z, tok[:, b0:e0].cpu().numpy().reshape(-1)).reshape(B, l)
        got = r.logp_drawn[:, b0:e0].cpu().numpy().astype(np.float64)
        err, bar = np.abs(got - want), R.lp_bound(want, V)
        worst = max(worst, float((err / bar).max()))
        assert (err <= bar).all(), (si, float(err.max()), float(bar.min()))
        assert (r.kept[:, b0:e0] == V).all()
    print(f'logp_drawn vs float64: worst error / bound {worst:.3f}')


def test_a_request_does_not_depend_on_its_neighbours():
    vae, var = _model()
    V = var.V
    sched = lambda lo, hi: np.linspace(lo, hi, S)[:, None]
    mine = dict(cfg=sched(0.5, 3.0), top_k=np.asarray([0, 0, 50, 900, 600])[:, None], top_p=sched(0.0, 0.9), temperature=sched(1.5, 0.6),
                min_p=sched(0.2, 0.0), logit_bias=np.stack([_bias(V, 10 + s) for s in range(S)])[:, None])
    alone = var.sample_controlled([980], [3], cfg_ramp=False, **mine)
    B = 3
    rng = np.random.default_rng(1)
    full = dict(cfg=np.broadcast_to(rng.uniform(0, 4, (S, B)), (S, B)).copy(), top_k=rng.integers(0, 1000, (S, B)), top_p=rng.uniform(0, 1, (S, B)),
                temperature=rng.uniform(0.5, 2.0, (S, B)), min_p=rng.uniform(0, 0.3, (S, B)),
                logit_bias=np.stack([_bias(V, 100 + i) for i in range(S * B)]).reshape(S, B, V))
    for k in full:
        full[k][:, 1] = mine[k][:, 0]
    among = var.sample_controlled([3, 980, 22], [17, 3, 5], cfg_ramp=False, **full)
    for k in FIELDS:
        assert torch.equal(_bits(getattr(alone, k)[0]), _bits(getattr(among, k)[1])), f'{k} of the request changed with its neighbours'
    assert len({tuple(t.tolist()) for t in among.tokens}) == B


def test_a_schedule_equals_hand_built_per_scale_kernel_calls():
    """(S, 1) schedules of every knob: each scale's tokens are those of varhip_ctl_sample_rows_f32 called by hand on that scale's logits with
    that scale's values and the Philox fill of (seed, scale)"""
    from var_amd import hip
    vae, var = _model()
    V, B = var.V, 3
    labels, seeds = [3, 980, 22], [17, 3, 5]
    cfgs, ks, ps = [0.0, 1.0, 2.5, 1.5, 4.0], [0, 5, 900, 0, 300], [0.0, 0.0, 0.96, 0.5, 0.0]
    taus, mps = [2.0, 1.0, 0.7, 1.3, 0.9], [0.0, 0.3, 0.0, 0.05, 0.1]
    bias = np.stack([_bias(V, 20 + s, bans=s % 2 == 0) for s in range(S)])
    col = lambda v: np.asarray(v)[:, None]
    kw = dict(cfg=col(cfgs), top_k=col(ks), top_p=col(ps), temperature=col(taus), min_p=col(mps), logit_bias=bias[:, None], cfg_ramp=False)
    r = var.sample_controlled(labels, seeds, decode=False, **kw)
    tok, st, logits, tab = _traced(var, labels, seeds, **kw)
    assert torch.equal(tok, r.tokens)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sd = dev(np.asarray(seeds, np.int64))
    for si, (b0, e0) in enumerate(var.begin_ends):
        l = e0 - b0
        noise = torch.empty(B * l, V, device='cuda')
        util.guarded_call('exp1_philox_f32', sd, B, l, V, si, 0, noise)
        idx = torch.full((B * l,), -7, dtype=torch.int64, device='cuda')
        masked = torch.empty(B * l, V, device='cuda')
        util.guarded_call('ctl_sample_rows_f32', logits[si].reshape(2 * B * l, V).contiguous(), noise, idx, masked, B, l, V, dev(np.full(B, cfgs[si])),
                          dev(np.full(B, ks[si], np.int32)), dev(np.full(B, ps[si])), dev(np.full(B, taus[si], np.float32)),
                          dev(np.full(B, mps[si], np.float32)), dev(bias[si]), dev(np.zeros(B, np.int32)), 1, V, ks[si] if ks[si] > 0 else V)
        assert torch.equal(idx.view(B, l), r.tokens[:, b0:e0]), f'scale {si}: the hand-built call drew other tokens'
        kept = (masked != float('-inf')).sum(-1).view(B, l).to(torch.int32)
        assert torch.equal(kept, r.kept[:, b0:e0]), f'scale {si}: kept'
    assert hip.lib() is not None


def test_ban_and_greedy_identities():
    vae, var = _model()
    d = DECK
    codes = [5, 4095, 1234, 0]
    bias = np.full((4, var.V), -np.inf, np.float32)
    bias[np.arange(4), codes] = 0.0
    r = var.sample_controlled(d['labels'], d['seeds'], cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'], temperature=[1.0, 0.7, 2.0, 1.0],
                              logit_bias=bias, decode=False)
    assert torch.equal(r.tokens.cpu(), torch.tensor(codes)[:, None].expand(4, var.L))
    assert bool((r.kept == 1).all()) and bool((r.logp_drawn == 0).all())
    a = var.sample_controlled(d['labels'], d['seeds'], cfg=d['cfg'], min_p=1.0, temperature=[1.0, 0.5, 3.0, 1.0])
    b = var.sample_controlled(d['labels'], d['seeds'], cfg=d['cfg'], top_k=1)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(_bits(a.images), _bits(b.images))
    assert bool((a.kept == 1).all()) and bool((b.kept == 1).all())


def test_hip_tokens_equal_the_pytorch_twin():
    """on the fixture configuration of tests/test_per_image_gpu.py (patch_nums (1, 2, 3, 4)), where the plain per-image call's tokens on HIP and
    in PyTorch are both shown equal to the oracle's"""
    pns = (1, 2, 3, 4)
    _, var = _model(pns)
    _, cpu = _model(pns, 'cpu')
    d = DECK
    kw = dict(cfg=d['cfg'], top_k=d['top_k'], top_p=d['top_p'])
    for extra in (dict(), dict(temperature=[0.7, 1.0, 1.0, 1.6], min_p=[0.0, 0.1, 0.0, 0.02], logit_bias=np.stack([_bias(var.V, 40 + i) for i in range(4)]))):
        g = var.sample_controlled(d['labels'], d['seeds'], decode=False, **kw, **extra)
        c = cpu.sample_controlled(d['labels'], d['seeds'], decode=False, **kw, **extra)
        assert torch.equal(g.tokens.cpu(), c.tokens), (sorted(extra), g.tokens.cpu(), c.tokens)
