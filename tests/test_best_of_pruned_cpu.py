"""VAR.sample_best_of_pruned without a GPU: the `keep` normalisation it shares with classify, the ABI entry of
varhip_kv_compact (its place in the tables and the Makefile), the refusal on a CPU model, and the pruning rule stated in numpy on a hand-made
per-token statistics array (what tests/test_best_of_pruned_gpu.py applies to the candidates' own per-image records)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests.util import ROOT
from var_amd.models.var import classify_rule, normalize_keep, rule_order


def best_of_rule(stats: np.ndarray, ends, schedule):
    """the rule of sample_best_of_pruned on full per-token statistics (B, n, L) fp32 of the field the call ranks by -> (choice, totals, depth):
    classify's rule on those scores (classify_rule: float64 running totals in token order, rule_order at every boundary and at the end)"""
    pred, total, depth, _ = classify_rule(stats, ends, schedule)
    return pred, total, depth


def test_keep_normalisation():
    assert normalize_keep(None, 5, 8) == [] and normalize_keep({}, 5, 8) == []
    assert normalize_keep({3: 2, 1: 4}, 5, 8) == [(1, 4), (3, 2)]                       # ascending in the scale
    assert normalize_keep({np.int64(3): np.int32(2), 0: 8}, 5, 8) == [(3, 2)]           # m == the survivor count: no boundary
    assert normalize_keep({0: 9, 1: 3, 2: 3, 3: 5}, 5, 8) == [(1, 3)]                   # drops nothing / nothing more: vanish
    assert normalize_keep({2: 1}, 5, 1) == []
    for bad in ([(1, 2)], 'x', {4: 2}, {-1: 2}, {1.0: 2}, {True: 2}, {'1': 2}, {1: 0}, {1: -3}, {1: 2.0}, {1: True}, {1: None}):
        with pytest.raises(ValueError, match='keep'):
            normalize_keep(bad, 5, 8)
    with pytest.raises(ValueError):
        normalize_keep({0: 1}, 1, 8)                                                      # one scale: no boundary exists


def test_kv_compact_in_header_abi_and_makefile():
    """(its argument list: tests/test_abi_cpu.py, for every declaration of the header)"""
    from var_amd import abi
    assert 'kv_compact' in abi.SIGNATURES_HIP_ONLY
    mk = open(os.path.join(ROOT, 'var_amd', 'csrc', 'Makefile')).read()
    assert 'kvcompact.hip' in mk.split('SRCS16')[0] and 'kvcompact' in mk.split('CHECKED')[1].split('\n')[0]


def test_cpu_model_is_refused_like_sample_best_of():
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        _, cpu = build_vae_var(device='cpu', patch_nums=(1, 2), depth=2, ch=32)
    cpu.eval()
    for call in (lambda: cpu.sample_best_of([3], [[1, 2]]), lambda: cpu.sample_best_of_pruned([3], [[1, 2]], {0: 1})):
        with pytest.raises(RuntimeError, match='HIP kernels only'):
            call()


def test_rule_on_a_hand_made_stats_array():
    """3 scales of 1, 2, 3 tokens (ends 1, 3, 6), two images of 5 candidates, schedule [(0, 4), (1, 2)]"""
    nan, f = np.float32('nan'), np.float32
    ends, L = [1, 3, 6], 6
    st = np.zeros((2, 5, L), np.float32)
    # image 0.  Scale 0: candidate 1 is NaN (below everything, -inf included), 3 holds -inf: the best 4 are {0, 2, 3, 4}, 1 is dropped at depth 0.
    st[0, :, 0] = [-1.0, nan, -2.0, -np.inf, -3.0]
    # scale 1: totals 0: -1 + (0.5 + -0.5) = -1;  2: -2 + 1 + 0 = -1 (an exact tie with 0: the lower index first);  3: -inf;  4: -3 + 2.5 + 0 = -0.5
    st[0, 0, 1:3] = [0.5, -0.5]; st[0, 2, 1:3] = [1.0, 0.0]; st[0, 3, 1:3] = [5.0, 5.0]; st[0, 4, 1:3] = [2.5, 0.0]
    # the best 2: 4 (-0.5), then 0 before 2 on the tie -> survivors {0, 4}; 2 and 3 end at depth 1
    st[0, 0, 3:] = [-1.0, -1.0, -1.0]          # -4
    st[0, 4, 3:] = [-1.0, -1.0, -1.5]          # -4: the final tie again goes to the lower index, 0
    st[0, 1, 1:] = 7.0; st[0, 2, 3:] = 7.0; st[0, 3, 3:] = 7.0        # what dropped candidates would have drawn is never read
    # image 1.  Scale 0: a +0 / -0 tie between 0 and 1 (equal totals: lower index first), 2 and 3 below them, 4 lowest: dropped.
    st[1, :, 0] = [0.0, -0.0, -1.0, -1.0, -5.0]
    # scale 1: 0: 0 - 8 = -8;  1: -0 + 0 + -0 stays a zero;  2: -1 + 1 + 0 = 0 (ties with candidate 1's zero: 1 first);  3: -1 - 1 = -2
    st[1, 0, 1:3] = [-4.0, -4.0]; st[1, 1, 1:3] = [0.0, -0.0]; st[1, 2, 1:3] = [1.0, 0.0]; st[1, 3, 1:3] = [-0.5, -0.5]
    # survivors {1, 2}.  Last scale: 1 turns NaN, 2 stays finite -> 2 wins
    st[1, 1, 3:] = [1.0, nan, 1.0]; st[1, 2, 3:] = [-1.0, -1.0, -1.0]
    choice, totals, depth = best_of_rule(st, ends, [(0, 4), (1, 2)])
    assert choice.tolist() == [0, 2]
    assert depth.tolist() == [[2, 0, 1, 1, 2], [1, 2, 2, 1, 0]]
    want0 = [-4.0, nan, -1.0, -np.inf, -4.0]
    assert np.array_equal(totals[0], np.asarray(want0), equal_nan=True) and totals.dtype == np.float64
    assert totals[1, 0] == -8.0 and np.isnan(totals[1, 1]) and totals[1, 2] == -3.0 and totals[1, 3] == -2.0 and totals[1, 4] == -5.0
    # the totals are running sums in token order (float64 additions of the fp32 values), not pairwise or fp32 sums
    big = np.zeros((1, 2, L), np.float32); big[0, 0] = [1e8, 1.0, -1e8, 1.0, 1.0, 1.0]; big[0, 1] = 3.0
    c, t, d = best_of_rule(big, ends, [])
    run = 0.0
    for v in big[0, 0]:
        run = run + float(v)
    assert t[0, 0] == run == 4.0 and c.tolist() == [1] and d.tolist() == [[2, 2]]
    # rule_order itself on the three special cases
    assert rule_order(np.asarray([nan, -np.inf, 1.0])).tolist() == [2, 1, 0]
    assert rule_order(np.asarray([-0.0, 0.0, 0.0])).tolist() == [0, 1, 2]
    assert rule_order(np.asarray([2.0, 3.0, 3.0, 2.0])).tolist() == [1, 2, 0, 3]
