"""History independence of VAR.sample_controlled, with the helpers of tests/test_call_order_gpu.py: a handful of
controlled calls, each alone on a fresh model, then interleaved with plain, per-image and composed calls in several orders on one model; every
result must be the bits of the same call made first on a fresh model.  One more pass runs with every workspace the engines keep overwritten
before each call."""
import collections

import numpy as np
import pytest
import torch

from tests import test_call_order_gpu as co

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}
SEEDS = [101, 7, (1 << 40) + 3]
S, V = 5, 4096


def _bias(seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((3, V)).astype(np.float32)
    b[:, rng.permutation(V)[:1000]] = -np.inf
    return b


def _lab():
    return torch.tensor(co.labels_of(3))


def ctl_default(vae, var):
    return co.record_fields(var.sample_controlled(_lab(), SEEDS, cfg=[1.5, 0.0, 4.0], top_k=[900, 0, 50], top_p=[0.96, 0.0, 0.5]))


def ctl_all(vae, var):
    return co.record_fields(var.sample_controlled(_lab(), SEEDS, cfg=[1.5, 0.0, 4.0], top_k=[900, 0, 50], top_p=[0.96, 0.0, 0.5], temperature=[0.7, 1.0, 1.8],
                                                  min_p=[0.05, 0.2, 0.0], logit_bias=_bias(1)))


def ctl_schedule(vae, var):
    col = lambda lo, hi: np.linspace(lo, hi, S)[:, None]
    r = var.sample_controlled(_lab(), SEEDS, cfg=col(0.0, 3.0), top_k=np.asarray([0, 0, 9, 900, 600])[:, None], top_p=col(0.0, 0.9), temperature=col(1.6, 0.6),
                              min_p=col(0.1, 0.0), logit_bias=_bias(2)[0], cfg_ramp=False, decode=False)
    return co.record_fields(r)


def composed(vae, var):
    r = var.sample_composed([[3, 5], [7, 9]], [[0.5, 0.5], [1.3, -0.3]], [31, 32], cfg=1.5, top_k=900, top_p=0.96)
    return dict(img=r.images, tokens=r.tokens, logp_class=r.logp_class, logp_drawn=r.logp_drawn)


DECK = [Entry('ctl default', 'f32', False, ctl_default, None), Entry('ar', 'f32', False, co.ar(2, 5), None), Entry('ctl all bf16', 'bf16', False, ctl_all, None),
        Entry('per image', 'f32', False, co.per_image, None), Entry('ctl schedule', 'f32', False, ctl_schedule, None), Entry('composed', 'f32', False, composed, None),
        Entry('ctl all f16', 'f16', False, ctl_all, None), Entry('ctl all', 'f32', False, ctl_all, None), Entry('per image scored', 'f32', False, co.per_image_scored, None)]
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


def test_the_controlled_calls_alone_differ_from_each_other():
    """the calls the other tests compare: the controls must act, or the orders below show nothing"""
    a, b = alone(DECK[0]), alone(DECK[7])
    assert not torch.equal(a['tokens'], b['tokens']) and bool((b['kept'] < a['kept']).any())
    assert torch.equal(a['tokens'], alone(DECK[8])['tokens'])


@pytest.mark.parametrize('order', [list(range(N)), list(reversed(range(N))), [3, 0, 5, 2, 1, 6, 4, 7, 8, 0, 7]], ids=['listed', 'reverse', 'mixed'])
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
    run_order([3, 0, 5, 2, 1, 6, 4, 7, 8, 0, 7], before_each)
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'
