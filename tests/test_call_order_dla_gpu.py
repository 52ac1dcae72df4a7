"""Call-order independence of VAR.logit_attribution (tests/test_call_order_gpu.py has the method): alone on a fresh model, interleaved with
evaluate, logit_lens and patch_effects in two orders, and once more with every workspace poisoned, a call's values are the bits it gives as the
first call on a fresh model."""
import collections

import pytest
import torch

from tests import test_call_order_gpu as co
from tests.test_call_order_lens_gpu import lens

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}
FIELDS = ('value', 'konst', 'embed', 'rest', 'residual', 'attn', 'mlp', 'attn_bias', 'head', 'rival')


def dla(N, target, layers, max_rows):
    def fn(vae, var):
        r = var.logit_attribution(co.eval_tokens(N, var.L), torch.tensor(co.labels_of(N)), target=target, layers=layers, max_rows=max_rows)
        return {k: getattr(r, k) for k in FIELDS}
    return fn


def patch_effects(vae, var):
    r = var.patch_effects(co.eval_tokens(2, var.L), torch.tensor(co.labels_of(2)), (('head', 0, 1), ('mlp', 1)), mode='mean', max_rows=3)
    return dict(nll=r.nll, entropy=r.entropy, kl=r.kl, pred=r.pred, rank=r.rank)


def refused(vae, var):
    var.logit_attribution(co.eval_tokens(2, var.L), torch.tensor(co.labels_of(2)))


DECK = [Entry('dla', 'f32', False, dla(5, 'gt', None, 4), None), Entry('evaluate', 'f32', False, co.evaluate(5, 2), None),
        Entry('dla margin one layer', 'f32', False, dla(3, 'margin', (1,), 64), None), Entry('lens', 'f32', False, lens(5, None, 4), None),
        Entry('patch effects', 'f32', False, patch_effects, None), Entry('dla refused bf16', 'bf16', False, refused, ValueError),
        Entry('dla one row', 'f32', False, dla(2, 'margin', None, 1), None)]
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


def test_the_alone_call_reads_the_real_logit():
    """the call the other tests compare: its value must be finite and its residual small, or the orders below show nothing"""
    a = alone(DECK[0])
    assert bool(torch.isfinite(a['head']).all()) and float(a['residual'].abs().max()) < 1e-2 and bool((a['rival'] == -1).all())
    assert bool((alone(DECK[2])['rival'] >= 0).all())


@pytest.mark.parametrize('order', [list(range(N)), [6, 4, 0, 3, 5, 2, 1, 0, 6]], ids=['listed', 'mixed'])
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
    run_order([6, 4, 0, 3, 5, 2, 1, 0, 6], before_each)
    assert max(written) >= 10, 'the poisoned pass found no workspace to poison'      # (this deck keeps one f32 teacher-forced set: 18 tensors)
