"""Call-order independence of VAR.attention_knockout (tests/test_call_order_gpu.py has the method): interleaved with sampling, evaluate, the
logit lens, patch_effects and a precision switch there and back, in two orders and once more with every workspace poisoned, a call's values are
the bits it gives as the first call on a fresh model."""
import collections

import pytest
import torch

from tests import test_call_order_gpu as co
from tests.test_call_order_patch_gpu import lens, patch

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}
EDGES = ((1, 0), (2, 2), ((2, 0), (2, 1)), (2, 1, 1), (1, 0, 0, 1))


def knockout(N, max_rows, edges=EDGES, **kw):
    def fn(vae, var):
        r = var.attention_knockout(co.eval_tokens(N, var.L), torch.tensor(co.labels_of(N)), edges, max_rows=max_rows, **kw)
        return dict(nll=r.nll, entropy=r.entropy, kl=r.kl, pred=r.pred, rank=r.rank)
    return fn


def refused(vae, var):
    var.attention_knockout(co.eval_tokens(2, var.L), torch.tensor(co.labels_of(2)), EDGES)


DECK = [Entry('knockout', 'f32', False, knockout(5, 64), None), Entry('ar', 'f32', False, co.ar(2, 5), None),
        Entry('knockout chunked', 'f32', False, knockout(3, 3), None), Entry('evaluate', 'f32', False, co.evaluate(5, 2), None),
        Entry('knockout one layer', 'f32', False, knockout(4, 7, EDGES[:3], layers=(1,), heads=(0,)), None), Entry('lens', 'f32', False, lens, None),
        Entry('patch zero', 'f32', False, patch(3, 'zero', 3), None), Entry('evaluate bf16', 'bf16', False, co.evaluate(5, 2), None),
        Entry('knockout refused f16', 'f16', False, refused, ValueError)]
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


def test_the_alone_knockout_starts_in_evaluate():
    """the call the other tests compare: its clean row must be evaluate's nll, or the orders below show nothing"""
    a, ev = alone(DECK[0]), alone(DECK[3])
    assert torch.equal(a['nll'][:, 0].view(torch.int32), ev['nll_BL'].view(torch.int32)) and not bool(a['kl'][:, 0].any()) and bool(a['kl'][:, 1:].any(-1).all())


@pytest.mark.parametrize('order', [list(range(N)), [7, 0, 3, 2, 6, 5, 4, 1, 8, 0, 2, 4]], ids=['listed', 'mixed'])
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
    run_order([7, 0, 3, 2, 6, 5, 4, 1, 8, 0, 2, 4], before_each)
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'
