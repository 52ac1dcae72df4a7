"""VAR.sample_composed without a GPU: the coefficient table against the float64 formula entry by entry, the argument checks,
and the numpy float32 twin of the mix that the GPU tests compare the kernel with (`mix_rows`: the operation order of
varhip_mix_sample_rows_f32, every product, sum and difference rounded to fp32 on its own)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import samplestatsref as R
from var_amd.engine import compose_tables, per_image_tables
from var_amd.models import args as A

F = np.float32


def mix_rows(logits, coef):
    """the mixed rows of one scale: logits (G, B, l, V) fp32, group-major with the unconditional group last; coef (B, G) fp32 ->
    (B * l, V) fp32:  acc = a_1*c_1;  acc = acc + a_k*c_k for k = 2 .. K;  x = acc - a_u*u   (numpy rounds every fp32 operation once)"""
    logits, coef = np.asarray(logits, F), np.asarray(coef, F)
    G, B, l, V = logits.shape
    a = [coef[:, g].reshape(B, 1, 1) for g in range(G)]
    with np.errstate(invalid='ignore', over='ignore'):
        acc = (a[0] * logits[0]).astype(F)
        for k in range(1, G - 1):
            p = (a[k] * logits[k]).astype(F)
            acc = (acc + p).astype(F)
        b = (a[G - 1] * logits[G - 1]).astype(F)
        return (acc - b).astype(F).reshape(B * l, V)


def t_of(cfg, si, S):
    return float(cfg) * (si / (S - 1)) if S > 1 else 0.0


# ---- the coefficient table --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [4, 10, 1])
def test_one_class_of_weight_one_gives_the_two_scalars_of_the_rows_entry(S):
    cfgs = [0, 1.5, 4, 0.1]
    coef = compose_tables(cfgs, np.ones((S, len(cfgs), 1)), S)
    assert coef.dtype == np.float32 and coef.shape == (S, len(cfgs), 2)
    tab = per_image_tables(cfgs, [0] * 4, [0.0] * 4, S, 4096)['t']
    for si in range(S):
        for b, cfg in enumerate(cfgs):
            t = t_of(cfg, si, S)
            assert t == tab[si][b]
            want = (np.float32(1 + t), np.float32(t))
            assert coef[si, b, 0].tobytes() == want[0].tobytes() and coef[si, b, 1].tobytes() == want[1].tobytes(), (si, cfg, coef[si, b], want)


def test_general_entries_are_the_float64_formula_rounded_once():
    S, B, K = 5, 6, 4
    rng = np.random.default_rng(3)
    w = rng.standard_normal((S, B, K)) * 2
    w[0, 0] = 0.0; w[1, 1, 2] = 0.0; w[2, 2] = [0.5, 0.5, 0.0, -1.25]; w[3, 3] = [1e-30, -3.0, 7.0, 1 / 3]
    cfgs = [0.0, 1.5, 4.0, 0.1, 2.5, 1e-3]
    coef = compose_tables(cfgs, w, S)
    assert coef.shape == (S, B, K + 1)
    for si in range(S):
        for b in range(B):
            t = t_of(cfgs[b], si, S)
            W = 0.0
            for k in range(K):
                W = W + float(w[si, b, k])
                assert coef[si, b, k].tobytes() == np.float32((1 + t) * float(w[si, b, k])).tobytes(), (si, b, k)
            assert coef[si, b, K].tobytes() == np.float32(t + (1 + t) * (W - 1)).tobytes(), (si, b)


def test_the_weights_are_summed_in_index_order():
    """1e16 + 1 is 1e16 in float64: (1e16, 1, -1e16) sums to 0 in index order and (1e16, -1e16, 1) to 1; a sorted, pairwise or compensated
    sum gives the same number for both"""
    t = 1.5 * (1 / 2)
    coef = compose_tables([1.5, 1.5], np.array([[[1e16, 1.0, -1e16], [1e16, -1e16, 1.0]]] * 3), 3)
    assert coef[1, 0, 3] == np.float32(t + (1 + t) * (0.0 - 1)) and coef[1, 1, 3] == np.float32(t + (1 + t) * (1.0 - 1))
    assert coef[1, 0, 3] != coef[1, 1, 3]


def test_table_refuses_a_scale_count_that_is_not_the_models():
    with pytest.raises(ValueError):
        compose_tables([1.5], np.ones((3, 1, 2)), 4)
    with pytest.raises(ValueError):
        compose_tables([1.5, 1.0], np.ones((4, 1, 2)), 4)


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------
GOOD = dict(labels=[[1, 2], [3, 1000]], weights=[[0.5, 0.5], [2.0, -1.0]], g_seeds=[5, 6], cfg=1.5, top_k=0, top_p=0.0, max_rows=128)
S_ARGS, NUM_CLASSES, V_ARGS = 4, 1000, 4096
REFUSED = {
    'K = 0': dict(labels=[[], []], weights=[[], []]),
    'K = 9': dict(labels=[list(range(9))] * 2, weights=[[1.0] * 9] * 2),
    'a NaN weight': dict(weights=[[0.5, float('nan')], [1.0, 1.0]]),
    'an infinite weight': dict(weights=[[0.5, 0.5], [float('inf'), 1.0]]),
    'a label above num_classes': dict(labels=[[1, 2], [3, 1001]]),
    'a negative label': dict(labels=[[1, -1], [3, 4]]),
    'float labels': dict(labels=[[1.0, 2.0], [3.0, 4.0]]),
    'labels (B,)': dict(labels=[1, 2]),
    'weights (K,)': dict(weights=[0.5, 0.5]),
    'weights (B, K + 1)': dict(weights=[[0.5, 0.5, 0.0]] * 2),
    'weights (B + 1, K)': dict(weights=[[0.5, 0.5]] * 3),
    "weights (S', B, K) with S' = S - 1": dict(weights=[[[0.5, 0.5]] * 2] * (S_ARGS - 1)),
    "weights (S', B, K) with S' = S + 1": dict(weights=[[[0.5, 0.5]] * 2] * (S_ARGS + 1)),
    'weights that are no numbers': dict(weights=[['a', 'b'], ['c', 'd']]),
    'one seed for two images': dict(g_seeds=[5]),
    'a negative seed': dict(g_seeds=[5, -1]),
    'top_k above V': dict(top_k=[0, V_ARGS + 1]),
    'top_p above 1': dict(top_p=1.5),
    'a NaN cfg': dict(cfg=float('nan')),
    'max_rows below one image': dict(max_rows=2),
    'max_rows that is no integer': dict(max_rows=7.5),
}


def _args(**over):
    kw = {**GOOD, **over}
    return A.compose_args(V_ARGS, NUM_CLASSES, S_ARGS, kw['labels'], kw['weights'], kw['g_seeds'], kw['cfg'], kw['top_k'], kw['top_p'], kw['max_rows'])


def test_good_arguments_are_normalised():
    lab, w, seeds, cfgs, ks, ps = _args()
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, 2) and w.dtype == np.float64 and w.shape == (S_ARGS, 2, 2)
    assert np.array_equal(w[0], w[3]) and w[1, 1].tolist() == [2.0, -1.0]
    assert (seeds, cfgs, ks, ps) == ([5, 6], [1.5, 1.5], [0, 0], [0.0, 0.0])
    per_scale = np.arange(S_ARGS * 4, dtype=np.float32).reshape(S_ARGS, 2, 2)
    assert np.array_equal(_args(weights=torch.from_numpy(per_scale))[1], per_scale.astype(np.float64))
    assert tuple(_args(labels=torch.tensor([[7]] * 2), weights=np.ones((2, 1)), max_rows=2)[0].shape) == (2, 1)
    assert tuple(_args(labels=[list(range(8))] * 2, weights=np.zeros((2, 8)))[0].shape) == (2, 8)


@pytest.mark.parametrize('what', sorted(REFUSED))
def test_refusals(what):
    with pytest.raises(ValueError):
        _args(**REFUSED[what])


def test_a_model_off_the_gpu_checks_its_arguments_and_then_refuses_as_the_scored_calls_do():
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        _, cpu = build_vae_var(device='cpu', patch_nums=(1, 2), depth=2, ch=32)
    cpu.eval()
    with pytest.raises(ValueError):
        cpu.sample_composed([[1, 2]], [[0.5, float('nan')]], [3])
    with pytest.raises(ValueError):
        cpu.sample_composed([[1, 2]], [[[0.5, 0.5]]] * 3, [3])          # S' = 3 on a model of two scales
    with pytest.raises(RuntimeError, match='HIP kernels only'):
        cpu.sample_composed([[1, 2]], [[0.5, 0.5]], [3])


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
def test_twin_with_two_groups_is_the_cfg_expression_and_keeps_a_row_under_one_and_zero():
    rng = np.random.default_rng(11)
    B, l, V = 3, 2, 256
    logits = (rng.standard_normal((2, B, l, V)) * 3).astype(F)
    ts = np.array([0.0, 1.5 * (1 / 9), 4.0 * (7 / 9)])
    coef = np.stack(((1.0 + ts).astype(F), ts.astype(F)), axis=1)
    assert np.array_equal(mix_rows(logits, coef).view(np.uint32), R.guided_rows(logits.reshape(2 * B * l, V), B, l, ts).view(np.uint32))
    m = mix_rows(logits, coef)
    pair = np.stack((m.reshape(B, l, V), np.zeros((B, l, V), F)))
    assert np.array_equal(mix_rows(pair, np.array([[1.0, 0.0]] * B, F)).view(np.uint32), m.view(np.uint32))     # 1*m - 0*0 = m, bit for bit


def test_twin_rounds_every_operation_on_its_own():
    """three groups on one element where each rounding shows: a fused multiply-add, or a float64 accumulator rounded at the end, gives another
    fp32 number"""
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 in fp32 (a tie, to even); minus 1 + 2^-11 that is 0, exactly 2^-24 without the rounding
    c = np.array([1 + 2.0 ** -12, 1 + 2.0 ** -11, 0.0], F).reshape(3, 1, 1, 1)
    a = np.array([[1 + 2.0 ** -12, -1.0, 1.0]], F)
    got = mix_rows(np.broadcast_to(c, (3, 1, 1, 256)).copy(), a)[0, 0]
    assert got == 0.0
    p1, p2, p3 = F(a[0, 0] * c[0, 0, 0, 0]), F(a[0, 1] * c[1, 0, 0, 0]), F(a[0, 2] * c[2, 0, 0, 0])
    assert got.tobytes() == F(F(p1 + p2) - p3).tobytes()
    exact = float(a[0, 0]) * float(c[0, 0, 0, 0]) + float(a[0, 1]) * float(c[1, 0, 0, 0]) - float(a[0, 2]) * float(c[2, 0, 0, 0])
    assert F(exact) != got, 'the example does not tell separate roundings from one rounding at the end'
