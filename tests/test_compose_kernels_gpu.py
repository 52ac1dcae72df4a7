"""varhip_mix_sample_rows_f32 on the MI355X.  Two groups with the coefficients ((float)(1 + t), (float)t): tokens and filtered
rows bit-equal to varhip_cfg_sample_rows_f32 on the same operands.  Three to five groups with positive, negative and zero coefficients: the
guided rows bit-equal to the numpy float32 twin (tests/test_compose_cpu.py::mix_rows), tokens and filtered rows bit-equal to
varhip_cfg_sample_rows_f32 run on (guided rows | zero rows) with t = 0 — 1 * m - 0 * 0 is m exactly, so the pinned kernel is the reference for
everything behind stage (1).  Both under either setting of varhip_sampler_force_walk, on dyadic logits with ties planted at the top-k
boundary, with every output pre-filled with a sentinel and every operand between guard bands.  Refused calls write nothing."""
import numpy as np
import pytest

from tests import util
from tests.test_compose_cpu import mix_rows

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(3, 1, 4096), (4, 9, 256), (2, 16, 8192), (2, 169, 1024)]
IDX_SENTINEL = -7
F = np.float32


def _hip():
    from var_amd import hip
    return hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _params(B, V):
    """per image (top_k, top_p), mixed, `none` included; top_k_cap as the engine forms it"""
    deck = [(0, 0.0), (min(900, V // 2), 0.96), (1, 0.0), (V // 4, 0.0), (0, 0.5), (V, 1.0)]
    ks, ps = [deck[b % len(deck)][0] for b in range(B)], [deck[b % len(deck)][1] for b in range(B)]
    return ks, ps, (V if 0 in ks else max(ks))


def _case(G, B, l, V, coef, ks, seed):
    """dyadic logits (multiples of 1/8 in [-8, 8)) [G, B, l, V] with ties planted where top-k cuts: in every row the column that holds the
    k-th largest mixed value is copied, in all groups, over three columns that held smaller values, so the k-th value is shared by at least
    four entries.  Noise: Exp(1)."""
    rng = np.random.default_rng(seed)
    logits = (rng.integers(-64, 64, size=(G, B, l, V)) / 8.0).astype(F)
    mixed = mix_rows(logits, coef).reshape(B, l, V)
    for b in range(B):
        k = ks[b] if 0 < ks[b] < V - 3 else max(1, V // 3)
        for t in range(l):
            order = np.argsort(-mixed[b, t], kind='stable')
            logits[:, b, t, order[-3:]] = logits[:, b, t, order[k - 1]][:, None]
    noise = rng.exponential(1.0, size=(B * l, V)).astype(F)
    return logits, noise


def _dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda', dt) if dt is not None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(B, l, V, guided=True):
    idx = torch.full((B * l,), IDX_SENTINEL, dtype=torch.int64, device='cuda')
    masked = torch.empty(B * l, V, device='cuda'); _bits(masked).fill_(-1)               # 0xFF bytes: a NaN the kernels never produce
    g = torch.empty(B * l, V, device='cuda') if guided else None
    if guided: _bits(g).fill_(-1)
    return idx, masked, g


def _untouched(idx, masked, g=None):
    return bool((idx == IDX_SENTINEL).all()) and bool((_bits(masked) == -1).all()) and (g is None or bool((_bits(g) == -1).all()))


def _rows_entry(logits2, noise, B, l, V, ts, ks, ps, cap):
    idx, masked, _ = _outputs(B, l, V, guided=False)
    util.guarded_call('cfg_sample_rows_f32', logits2, noise, idx, masked, B, l, V, _dev(np.asarray(ts, np.float64)), _dev(np.asarray(ks, np.int32)),
                      _dev(np.asarray(ps, np.float64)), cap)
    return idx, masked


@pytest.mark.parametrize('B, l, V', SHAPES)
def test_two_groups_are_the_rows_entry_bit_for_bit(B, l, V):
    """the test that catches a contracted fma or another operation order in stage (1): the coefficients are not dyadic, so every product rounds"""
    hip = _hip()
    ts = [0.0, 1.5 * (1 / 9), 4.0 * (7 / 9), 0.75][:B]
    coef = np.stack(((1.0 + np.asarray(ts)).astype(F), np.asarray(ts).astype(F)), axis=1)
    ks, ps, cap = _params(B, V)
    logits, noise = _case(2, B, l, V, coef, ks, seed=V + l)
    lg, nz, cf = _dev(logits.reshape(2 * B * l, V)), _dev(noise), _dev(coef)
    tk, tp = _dev(np.asarray(ks, np.int32)), _dev(np.asarray(ps, np.float64))
    try:
        for walk in (0, 1):
            hip.lib().so.varhip_sampler_force_walk(walk)
            idx, masked, g = _outputs(B, l, V)
            util.guarded_call('mix_sample_rows_f32', lg, nz, idx, masked, g, B, l, V, 2, cf, tk, tp, cap)
            want_idx, want_masked = _rows_entry(lg, nz, B, l, V, ts, ks, ps, cap)
            assert int(idx.min()) >= 0 and int(idx.max()) < V
            assert torch.equal(idx, want_idx), (walk, idx, want_idx)
            assert torch.equal(_bits(masked), _bits(want_masked)), walk
            assert np.array_equal(g.cpu().numpy().view(np.uint32), mix_rows(logits, coef).view(np.uint32)), walk
            idx2, masked2, _ = _outputs(B, l, V, guided=False)                                    # guided_out is optional
            util.guarded_call('mix_sample_rows_f32', lg, nz, idx2, masked2, None, B, l, V, 2, cf, tk, tp, cap)
            assert torch.equal(idx2, idx) and torch.equal(_bits(masked2), _bits(masked))
            idx3 = torch.full((B * l,), IDX_SENTINEL, dtype=torch.int64, device='cuda')          # ... and so is masked_out
            util.guarded_call('mix_sample_rows_f32', lg, nz, idx3, None, None, B, l, V, 2, cf, tk, tp, cap)
            assert torch.equal(idx3, idx)
    finally:
        hip.lib().so.varhip_sampler_force_walk(0)


COEFS = {           # per image: K class coefficients, then the unconditional one; positive, negative and zero, none of them dyadic but the zeros
    3: [[0.3, 1.7, 0.9], [1.1, -0.7, -0.6], [0.0, 2.3, 1.3], [1.9, 0.0, 0.0]],
    4: [[0.3, 0.45, 1.7, 1.45], [1.3, -0.7, 0.0, -0.4], [-0.2, 0.0, 2.9, 1.7], [0.0, 0.0, 0.0, -1.0]],
    5: [[0.3, 0.3, 0.3, 0.3, 0.2], [2.1, -0.7, 0.0, 1.3, 1.7], [0.0, 0.0, -1.1, 3.3, 1.2], [1e-3, -1e3, 1e3, 0.6, -0.4]],
}


@pytest.mark.parametrize('B, l, V', SHAPES)
@pytest.mark.parametrize('G', [3, 4, 5])
def test_more_groups_equal_the_twin_and_the_rows_entry_on_the_guided_rows(G, B, l, V):
    hip = _hip()
    coef = np.asarray(COEFS[G][:B], F)
    ks, ps, cap = _params(B, V)
    logits, noise = _case(G, B, l, V, coef, ks, seed=100 * G + l)
    want_g = mix_rows(logits, coef)
    lg, nz, cf = _dev(logits.reshape(G * B * l, V)), _dev(noise), _dev(coef)
    tk, tp = _dev(np.asarray(ks, np.int32)), _dev(np.asarray(ps, np.float64))
    try:
        for walk in (0, 1):
            hip.lib().so.varhip_sampler_force_walk(walk)
            idx, masked, g = _outputs(B, l, V)
            util.guarded_call('mix_sample_rows_f32', lg, nz, idx, masked, g, B, l, V, G, cf, tk, tp, cap)
            assert np.array_equal(g.cpu().numpy().view(np.uint32), want_g.view(np.uint32)), (walk, 'guided_out differs from the float32 twin')
            pair = torch.cat((g, torch.zeros_like(g)))
            want_idx, want_masked = _rows_entry(pair, nz, B, l, V, [0.0] * B, ks, ps, cap)
            assert int(idx.min()) >= 0 and int(idx.max()) < V
            assert torch.equal(idx, want_idx), (walk, idx, want_idx)
            assert torch.equal(_bits(masked), _bits(want_masked)), walk
            kept = (masked != float('-inf')).sum(-1).view(B, l)
            for b in range(B):                                   # the planted ties are there: top-k keeps more than k entries
                if 1 < ks[b] < V - 3 and ps[b] == 0.0:
                    assert int(kept[b].min()) >= ks[b] + 3, (b, ks[b], kept[b])
    finally:
        hip.lib().so.varhip_sampler_force_walk(0)


def test_an_image_with_a_bad_top_k_gets_minus_one_and_nothing_else():
    B, l, V, G = 3, 2, 1024, 3
    coef = np.asarray(COEFS[3][:B], F)
    logits, noise = _case(G, B, l, V, coef, [8, 900, 8], seed=5)
    for bad in (900, -1, V + 1):                                 # more than the launch's sort buffer holds; outside [0, V]
        idx, masked, g = _outputs(B, l, V)
        util.guarded_call('mix_sample_rows_f32', _dev(logits.reshape(-1, V)), _dev(noise), idx, masked, g, B, l, V, G, _dev(coef),
                          _dev(np.asarray([8, bad, 8], np.int32)), _dev(np.zeros(B)), 8)
        i2 = idx.view(B, l)
        assert bool((i2[1] == -1).all()) and int(i2[[0, 2]].min()) >= 0, (bad, idx)
        assert bool((_bits(masked).view(B, l, V)[1] == -1).all()) and bool((_bits(g).view(B, l, V)[1] == -1).all()), bad
        assert bool(torch.isfinite(g.view(B, l, V)[[0, 2]]).all()) and bool(((masked.view(B, l, V)[[0, 2]] != float('-inf')).sum(-1) >= 8).all())


def test_refused_calls_write_nothing():
    hip = _hip()
    from var_amd import abi
    B, l, V, G = 2, 3, 256, 3
    lg = torch.zeros(G * B * l * V + 4, device='cuda')
    nz = torch.ones(B * l, V, device='cuda')
    cf = torch.ones(B, G, device='cuda')
    tk = torch.zeros(B, dtype=torch.int32, device='cuda')
    tp = torch.zeros(B, dtype=torch.float64, device='cuda')
    gbuf = torch.empty(B * l * V + 4, device='cuda'); _bits(gbuf).fill_(-1)
    idx, masked, _ = _outputs(B, l, V, guided=False)
    fn, st = hip.lib().fn['mix_sample_rows_f32'], hip.current_stream()
    invoke = lambda *a: fn(*a, st)
    good = [lg[:G * B * l * V], nz, idx, masked, gbuf[:B * l * V], B, l, V, G, cf, tk, tp, V]
    bad = [(8, 1), (8, 0), (8, 10), (8, -3), (0, None), (1, None), (2, None), (9, None), (10, None), (11, None), (0, lg[1:G * B * l * V + 1]),
           (4, gbuf[1:B * l * V + 1]), (5, 0), (6, 0), (7, 0), (7, 255), (7, 260), (7, 8448), (12, 0), (12, V + 1)]
    for pos, val in bad:
        a = list(good); a[pos] = val
        rc = util.guarded_invoke('varhip_mix_sample_rows_f32', a, invoke, torch.cuda.synchronize)
        assert rc == abi.EINVAL, (pos, val, rc)
        assert _untouched(idx, masked, gbuf), (pos, val)
    with pytest.raises(hip.VarHipError, match='EINVAL'):
        hip.call('mix_sample_rows_f32', *[good[i] if i != 8 else 1 for i in range(len(good))])
    assert util.guarded_invoke('varhip_mix_sample_rows_f32', good, invoke, torch.cuda.synchronize) == 0          # the same operands, accepted
    assert int(idx.min()) >= 0 and not _untouched(idx, masked, gbuf)
