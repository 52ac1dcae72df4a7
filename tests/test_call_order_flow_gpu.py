"""Call-order independence of VAR.attention_maps and VAR.attention_rollout (tests/test_call_order_gpu.py has the method): alone on a fresh model,
interleaved with evaluate, attention_profile and logit_lens in two orders, and once more with every workspace poisoned, a call's values are the
bits it gives as the first call on a fresh model."""
import collections

import pytest
import torch

from tests import test_call_order_gpu as co
from tests.test_call_order_lens_gpu import lens

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}
TARGETS = (0, 3, (2, 1, 1), 29, (4, 4, 4))


def maps(N, layers, max_rows, targets=TARGETS):
    def fn(vae, var):
        r = var.attention_maps(co.eval_tokens(N, var.L), torch.tensor(co.labels_of(N)), targets, layers=layers, max_rows=max_rows)
        return dict(rows=r.rows, nan_queries=r.nan_queries)
    return fn


def rollout(N, layers, max_rows, alpha=0.5):
    def fn(vae, var):
        r = var.attention_rollout(co.eval_tokens(N, var.L), torch.tensor(co.labels_of(N)), TARGETS, layers=layers, alpha=alpha, max_rows=max_rows)
        return dict(flow=r.flow, nan_queries=r.nan_queries)
    return fn


def refused(vae, var):
    var.attention_rollout(co.eval_tokens(2, var.L), torch.tensor(co.labels_of(2)), TARGETS)


DECK = [Entry('maps', 'f32', False, maps(5, None, 4), None), Entry('evaluate', 'f32', False, co.evaluate(5, 2), None),
        Entry('rollout', 'f32', False, rollout(5, None, 2), None), Entry('lens', 'f32', False, lens(5, None, 4), None),
        Entry('attention profile', 'f32', False, co.attention_profile, None), Entry('rollout refused bf16', 'bf16', False, refused, ValueError),
        Entry('maps one layer one row', 'f32', False, maps(3, (1,), 1, (54,)), None), Entry('rollout one layer', 'f32', False, rollout(2, (0,), 8, 0.25), None)]
N = len(DECK)


def alone(e):
    if e.name not in _ALONE:
        vae, var = co.fresh('t')
        _ALONE[e.name] = co.run(e, vae, var)
    return _ALONE[e.name]


def shared():
    if 't' not in _SHARED:
        _SHARED['t'] = co.fresh('t')
    return _SHARED['t']


def run_order(order, before_each=None):
    bad, prev = [], '(nothing)'
    vae, var = shared()
    for i in order:
        e = DECK[i]
        want = alone(e)
        if before_each is not None:
            before_each()
        d = co.difference(co.run(e, vae, var), want)
        if d is not None:
            bad.append(f'{e.name} right after {prev}: {d}')
        prev = e.name
    assert not bad, '\n'.join(bad)


def test_the_alone_calls_see_real_attention():
    """the calls the other tests compare: finite, normalised rows, or the orders below show nothing"""
    a, r = alone(DECK[0]), alone(DECK[2])
    assert bool(torch.isfinite(a['rows']).all()) and float((a['rows'].double().sum(-1) - 1).abs().max()) < 1e-3 and not a['nan_queries'].any()
    assert bool(torch.isfinite(r['flow']).all()) and float((r['flow'].double().sum(-1) - 1).abs().max()) < 1e-3 and bool((r['flow'][:, 4] > 0).sum() > 5)


@pytest.mark.parametrize('order', [list(range(N)), [7, 4, 0, 3, 5, 2, 1, 6, 0, 2]], ids=['listed', 'mixed'])
def test_every_order_gives_the_alone_results(order):
    run_order(order)


def test_poisoned_workspaces_change_nothing():
    run_order(list(range(N)))                                # (run on its own: give the model a history first)
    written = []

    def before_each():
        torch.cuda.synchronize()
        written.append(co.poison_engines(*shared()))
        co.poison_allocator()
        torch.cuda.synchronize()
    run_order([7, 4, 0, 3, 5, 2, 1, 6, 0, 2], before_each)
    assert max(written) >= 10, 'the poisoned pass found no workspace to poison'
