"""History independence of VAR.abduct_noise and VAR.counterfactual, with the helpers of tests/test_call_order_gpu.py:
each call alone on a fresh model, then interleaved with plain, per-image and scored calls in several orders on one model; every result must be
the bits of the same call made first on a fresh model.  One more pass runs with every workspace the engines keep overwritten before each call."""
import collections

import torch
import pytest

from tests import test_call_order_gpu as co

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}
SEEDS = [101, 7, (1 << 40) + 3]
CFG = [1.5, 0.0, 4.0]


def _lab():
    return torch.tensor(co.labels_of(3))


def _tokens(var):
    """three legal token rows that depend on nothing but their index (no call is needed to make them)"""
    i = torch.arange(3 * var.L, dtype=torch.int64).view(3, var.L)
    return ((i * 2654435761 + 12345) % var.V).cuda()


def abduct(vae, var):
    r = var.abduct_noise(_tokens(var), _lab(), SEEDS, cfg=CFG, first_scale=1, max_images=2)
    return dict(noise=r.noise, logp_src=r.logp_src, unreachable=r.unreachable)


def counterfactual(vae, var):
    dst = torch.stack((_lab().flip(0), _lab()), dim=1)
    r = var.counterfactual(_tokens(var), _lab(), dst, SEEDS, cfg=CFG, cfg_dst=[3.0, 1.5, 0.0], top_k=[0, 900, 50], top_p=[0.0, 0.96, 0.5], first_scale=1,
                           max_images=4)
    return dict(images=r.images, tokens=r.tokens, changed=r.changed, first=r.first_changed_scale, logp_src=r.logp_src, **co.record_fields(r.record, 'rec_'))


DECK = [Entry('abduct', 'f32', False, abduct, None), Entry('ar', 'f32', False, co.ar(2, 5), None), Entry('counterfactual bf16', 'bf16', False, counterfactual, None),
        Entry('per image', 'f32', False, co.per_image, None), Entry('counterfactual', 'f32', False, counterfactual, None),
        Entry('abduct f16', 'f16', False, abduct, None), Entry('per image scored', 'f32', False, co.per_image_scored, None)]
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


def test_the_calls_alone_do_something():
    """the calls the other tests compare: the replay under other labels must move tokens, and its second column — the source's own labels with
    another cfg and filters — must differ from the first"""
    a = alone(DECK[4])
    assert bool(a['changed'].any()) and not torch.equal(a['tokens'][:, 0], a['tokens'][:, 1])
    assert bool(torch.isfinite(alone(DECK[0])['noise']).all())


@pytest.mark.parametrize('order', [list(range(N)), list(reversed(range(N))), [3, 0, 5, 2, 1, 6, 4, 0, 4]], ids=['listed', 'reverse', 'mixed'])
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
    run_order([3, 0, 5, 2, 1, 6, 4, 0, 4], before_each)
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'
