"""VAR.sample_controlled without a GPU: the host tables and their checkers, the identities of the call on a tiny CPU model
(the PyTorch twin), and the numpy restatement of the min-p stage (tests/ctlref.py) against float64."""
import contextlib
import io

import numpy as np
import pytest

from tests import ctlref

torch = pytest.importorskip('torch')

S, B, V = 5, 3, 4096
PNS, DEPTH, CH = (1, 2, 3), 2, 32
_M = {}


def _tables(**kw):
    from var_amd.engine import control_tables
    a = dict(cfg=1.5, top_k=0, top_p=0.0, temperature=1.0, min_p=0.0, logit_bias=None)
    a.update(kw)
    ramp = a.pop('cfg_ramp', True)
    return control_tables(a['cfg'], a['top_k'], a['top_p'], a['temperature'], a['min_p'], a['logit_bias'], S, V, B, ramp)


def _model():
    if 'm' not in _M:
        from models import build_vae_var
        from var_amd.detinit import fill_module_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=PNS, depth=DEPTH, ch=CH)
        fill_module_(var, DEPTH, 0, 'var.'); fill_module_(vae, DEPTH, 0, 'vae.')
        _M['m'] = (vae, var.eval())
    return _M['m']


# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
KNOBS = dict(cfg=('t', 2.5, np.float64), top_k=('top_k', 7, np.int32), top_p=('top_p', 0.5, np.float64), temperature=('tau', 0.7, np.float32),
             min_p=('min_p', 0.1, np.float32))


@pytest.mark.parametrize('knob', list(KNOBS))
def test_every_accepted_shape_broadcasts_to_S_B(knob):
    key, v, dt = KNOBS[knob]
    per_b = np.asarray([v, v / 2 if knob != 'top_k' else v + 1, v])
    per_s = np.arange(1, S + 1)[:, None] * (v / S if knob != 'top_k' else 1)
    full = per_s * np.ones((1, B))
    for given, want in [(v, np.full((S, B), v)), ([v], np.full((S, B), v)), (per_b, np.broadcast_to(per_b, (S, B))), (per_b.tolist(), np.broadcast_to(per_b, (S, B))),
                        (torch.from_numpy(per_b), np.broadcast_to(per_b, (S, B))), (per_s, np.broadcast_to(per_s, (S, B))), (full, full)]:
        tab = _tables(**{knob: given}, cfg_ramp=False) if knob == 'cfg' else _tables(**{knob: given})
        got = tab[key]
        assert got.shape == (S, B) and got.dtype == dt, (knob, got.shape, got.dtype)
        assert np.array_equal(got, np.asarray(want).astype(dt)), (knob, given)
    assert len(_tables()['cap']) == S


def test_cfg_ramp_reproduces_the_per_image_table_bit_for_bit():
    from var_amd.engine import per_image_tables
    cfgs = [1.5, 0.3, 4.1]
    want = per_image_tables(cfgs, [0] * B, [0.0] * B, S, V)['t']
    assert np.array_equal(_tables(cfg=cfgs)['t'].view(np.uint64), want.view(np.uint64))
    assert np.array_equal(_tables(cfg=1.5)['t'].view(np.uint64), per_image_tables([1.5] * B, [0] * B, [0.0] * B, S, V)['t'].view(np.uint64))
    assert np.array_equal(_tables(cfg=want, cfg_ramp=False)['t'].view(np.uint64), want.view(np.uint64))      # the same values, fed as a schedule
    one = per_image_tables([1.5], [0], [0.0], S, V)['t']
    assert np.array_equal(_tables(cfg=one, cfg_ramp=False)['t'], np.broadcast_to(one, (S, B)))                # (S, 1): a pure schedule


def test_cap_is_per_scale():
    k = np.full((S, B), 5); k[1, 2] = 900; k[3, 0] = 0
    assert _tables(top_k=k)['cap'] == [5, 900, 5, V, 5]


def test_bias_rows_are_deduplicated():
    rng = np.random.default_rng(0)
    r0, r1, r2 = (rng.standard_normal(V).astype(np.float32) for _ in range(3))
    r2[::2] = -np.inf
    t = _tables()
    assert t['bias'] is None and (t['bias_row'] == -1).all()
    t = _tables(logit_bias=r0)
    assert t['bias'].shape == (1, V) and (t['bias_row'] == 0).all() and t['bias_row'].dtype == np.int32
    t = _tables(logit_bias=np.stack([r0, r1, r0]))
    assert t['bias'].shape == (2, V) and np.array_equal(t['bias_row'], np.broadcast_to([0, 1, 0], (S, B)))
    assert np.array_equal(t['bias'][1], r1)
    t = _tables(logit_bias=r1[None])
    assert t['bias'].shape == (1, V) and (t['bias_row'] == 0).all()
    sched = np.stack([r0, r0, r1, r2, r0])[:, None]                                    # (S, 1, V)
    t = _tables(logit_bias=sched)
    assert t['bias'].shape == (3, V) and np.array_equal(t['bias_row'], np.broadcast_to(np.asarray([0, 0, 1, 2, 0])[:, None], (S, B)))
    full = np.broadcast_to(sched, (S, B, V)).copy(); full[4, 1] = r2
    t = _tables(logit_bias=full)
    assert t['bias'].shape == (3, V) and t['bias_row'][4].tolist() == [0, 2, 0] and t['bias'].dtype == np.float32
    assert np.array_equal(t['bias'][t['bias_row']].view(np.uint32), full.view(np.uint32))


# ---- the checkers -------------------------------------------------------------------------------------------------------------------------
def _bias(**edit):
    b = np.zeros(V, np.float32)
    for k, v in edit.items():
        b[int(k[1:])] = v
    return b


BAD = [('temperature', 0.0), ('temperature', -1.0), ('temperature', float('inf')), ('temperature', float('nan')), ('temperature', [1.0, 0.5, 1e-60]),
       ('temperature', np.ones((S + 1, B))), ('temperature', [1.0, 1.0]), ('temperature', 'hot'), ('temperature', True),
       ('min_p', -0.1), ('min_p', 1.01), ('min_p', float('nan')), ('min_p', np.zeros((B, S))),
       ('top_k', -1), ('top_k', V + 1), ('top_k', 1.5), ('top_k', np.zeros((S, 2))),
       ('top_p', -0.1), ('top_p', 1.5), ('top_p', float('nan')), ('top_p', np.zeros(S + 3)),
       ('cfg', float('inf')), ('cfg', np.zeros((2, 2, 2))),
       ('logit_bias', _bias(i3=float('nan'))), ('logit_bias', _bias(i3=float('inf'))), ('logit_bias', np.full(V, -np.inf, np.float32)),
       ('logit_bias', np.zeros(V - 1, np.float32)), ('logit_bias', np.zeros((B + 1, V), np.float32)), ('logit_bias', np.zeros((S - 1, B, V), np.float32)),
       ('logit_bias', np.stack([_bias(), np.full(V, -np.inf, np.float32), _bias()]))]


@pytest.mark.parametrize('i', range(len(BAD)))
def test_refusals_name_the_argument(i):
    name, val = BAD[i]
    with pytest.raises(ValueError, match=name):
        _tables(**{name: val})


def test_temperature_zero_points_to_top_k_1_and_shapes_are_named():
    with pytest.raises(ValueError, match='top_k=1'):
        _tables(temperature=0.0)
    with pytest.raises(ValueError, match=rf'\({S}, {B}\).*\(7, {B}\)'):
        _tables(min_p=np.zeros((7, B)))
    with pytest.raises(ValueError, match=rf'\({S}, {B}, {V}\).*\(2, {V}\)'):
        _tables(logit_bias=np.zeros((2, V), np.float32))


def test_the_public_call_checks_its_arguments():
    vae, var = _model()
    for bad in [dict(temperature=0.0), dict(min_p=2.0), dict(top_k=var.V + 1), dict(top_p=-1.0), dict(g_seeds=[1]), dict(label_B=[1, 1001]),
                dict(logit_bias=np.full(var.V, -np.inf, np.float32)), dict(cfg=[1.0, 2.0, 3.0])]:
        with pytest.raises(ValueError):
            var.sample_controlled(**{**dict(label_B=[1, 2], g_seeds=[0, 1]), **bad})


# ---- the call on the PyTorch twin ---------------------------------------------------------------------------------------------------------
LAB, SEEDS = [3, 980, 22], [17, 3, (1 << 62) + 5]


def test_a_ban_of_all_codes_but_one_makes_every_token_that_code():
    vae, var = _model()
    codes = [5, 4095, 1234]
    bias = np.full((3, var.V), -np.inf, np.float32)
    bias[np.arange(3), codes] = 0.0
    r = var.sample_controlled(LAB, SEEDS, cfg=[4.0, 1.5, 0.0], top_k=[0, 900, 0], top_p=[0.96, 0.0, 0.0], temperature=[1.0, 0.7, 2.0], logit_bias=bias)
    assert r.tokens.shape == (3, var.L) and r.images.shape == (3, 3, 48, 48)
    assert torch.equal(r.tokens, torch.tensor(codes)[:, None].expand(3, var.L))
    assert r.logp_drawn is None and 'no per-token statistics' in repr(r)


def test_min_p_one_is_greedy():
    vae, var = _model()
    a = var.sample_controlled(LAB, SEEDS, cfg=[4.0, 1.5, 0.0], min_p=1.0, temperature=[1.0, 0.5, 3.0])
    b = var.sample_controlled(LAB, SEEDS, cfg=[4.0, 1.5, 0.0], top_k=1)
    c = var.autoregressive_infer_cfg_per_image(LAB, SEEDS, cfg=[4.0, 1.5, 0.0], top_k=1, return_tokens=True)[1]
    assert torch.equal(a.tokens, b.tokens) and torch.equal(b.tokens, c)
    assert torch.equal(a.images, b.images)


def test_default_controls_are_the_per_image_call():
    vae, var = _model()
    kw = dict(cfg=[4.0, 1.5, 0.0], top_k=[0, 900, 1], top_p=[0.96, 0.0, 0.0])
    img, tok = var.autoregressive_infer_cfg_per_image(LAB, SEEDS, return_tokens=True, **kw)
    r = var.sample_controlled(LAB, SEEDS, **kw)
    assert torch.equal(r.tokens, tok) and torch.equal(r.images, img)
    assert var.sample_controlled(LAB, SEEDS, decode=False, **kw).images is None
    alone = var.sample_controlled(LAB[1:2], SEEDS[1:2], cfg=1.5, top_k=900, temperature=0.8, min_p=0.05)
    among = var.sample_controlled(LAB, SEEDS, cfg=[4.0, 1.5, 0.0], top_k=[0, 900, 1], temperature=[1.3, 0.8, 1.0], min_p=[0.0, 0.05, 0.5])
    assert torch.equal(alone.tokens[0], among.tokens[1])


# ---- the restatement against float64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Vr, js', [(256, (1, 2, 5, 17, 100, 255)), (4096, (1, 3, 10, 40))])
def test_min_p_restatement_leaves_exactly_j_codes(Vr, js):
    x, mp, want = ctlref.rows_with_known_survivors(2 * len(js), Vr, js, seed=Vr)
    for row, p, j in zip(x, mp, want):
        cut = ctlref.min_p_cut(row[None], p)[0]
        kept = cut > -np.inf
        assert int(kept.sum()) == j, (j, int(kept.sum()))
        assert np.array_equal(np.flatnonzero(kept), np.sort(np.argsort(-row.astype(np.float64), kind='stable')[:j]))
        assert np.array_equal(cut[kept].view(np.uint32), row[kept].view(np.uint32))
    assert np.array_equal(ctlref.min_p_cut(x, 0.0).view(np.uint32), x.view(np.uint32))
    one = ctlref.min_p_cut(x, 1.0)
    assert ((one > -np.inf).sum(-1) == 1).all() and np.array_equal(one.argmax(-1), x.argmax(-1))


def test_bias_and_temperature_restatement():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((4, 256)).astype(np.float32); x[0, 0] = -0.0
    b = rng.standard_normal(256).astype(np.float32); b[7] = -np.inf
    assert np.array_equal(ctlref.bias_temper(x).view(np.uint32), x.view(np.uint32))                  # neutral: not even -0 changes
    y = ctlref.bias_temper(x, b, 0.7)
    want = (x.astype(np.float64) + b.astype(np.float64)).astype(np.float32).astype(np.float64) / float(np.float32(0.7))
    assert np.array_equal(y, want.astype(np.float32)) and (y[:, 7] == -np.inf).all()
