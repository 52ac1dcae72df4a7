"""History independence of VAR.sample_smc, with the helpers of tests/test_call_order_gpu.py: the call alone on a fresh
model, then before and after autoregressive_infer_cfg, sample_best_of_pruned, token_log_likelihood and a precision switch, in several orders on
one model; every result must be the bits of the same call made first on a fresh model.  One more pass runs with every workspace the engines
keep (sample_smc's buffer set among them) overwritten before each call."""
import collections

import pytest
import torch

from tests import test_call_order_gpu as co

pytestmark = pytest.mark.gpu

KW = dict(cfg=1.5, top_k=900, top_p=0.96)
SEEDS = [[31, 32, 33, 34], [41, 42, 43, 44]]
Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}


def _lab():
    return torch.tensor(co.labels_of(2), device='cuda')


def smc(vae, var):
    r = var.sample_smc(_lab(), SEEDS, resample=(1, 3), beta=20.0, ess=None, **KW)
    out = dict(img=r.images, log_weights=r.log_weights, ancestors=r.ancestors, resampled=r.resampled, ess=r.ess, seen=r.log_weights_seen,
               **co.record_fields(r.particles))
    return {k: v for k, v in out.items() if v is not None}


def smc_threshold(vae, var):
    r = var.sample_smc(_lab(), SEEDS, resample=(0, 2), beta=1.0, ess=0.9, by='logp_drawn', max_images=4, decode=False, **KW)
    out = dict(log_weights=r.log_weights, ancestors=r.ancestors, resampled=r.resampled, **co.record_fields(r.particles))
    return {k: v for k, v in out.items() if v is not None}


def pruned(vae, var):
    r = var.sample_best_of_pruned(_lab(), SEEDS, {1: 3, 3: 1}, **KW)
    return dict(img=r.images, totals=r.totals, choice=r.choice, tokens=r.tokens)


DECK = [Entry('smc f32', 'f32', False, smc, None), Entry('ar', 'f32', False, co.ar(2, 5), None), Entry('smc bf16', 'bf16', False, smc, None),
        Entry('pruned', 'f32', False, pruned, None), Entry('smc threshold', 'f32', False, smc_threshold, None), Entry('loglik', 'f32', False, co.loglik, None),
        Entry('smc f16', 'f16', False, smc, None), Entry('pruned bf16', 'bf16', False, pruned, None)]


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


def test_sample_smc_alone_resamples():
    """the call the other tests compare: it must move particles, or the orders below show nothing"""
    r = alone(DECK[0])
    ident = torch.arange(4).expand_as(r['ancestors'])
    assert bool(r['resampled'].all()) and int((r['ancestors'] != ident).sum()) >= 1


@pytest.mark.parametrize('order', [list(range(8)), list(reversed(range(8))), [3, 0, 5, 2, 1, 6, 4, 7, 0]], ids=['listed', 'reverse', 'mixed'])
def test_every_order_gives_the_alone_results(order):
    run_order(order)


def test_poisoned_workspaces_change_nothing(monkeypatch):
    monkeypatch.setattr(co, 'POISONED', co.POISONED | {'SamplingEngine._ws_bop'})
    run_order(list(range(8)))                                # (run on its own: give the model a history first)
    written = []

    def before_each():
        torch.cuda.synchronize()
        written.append(co.poison_engines(*shared()))
        co.poison_allocator()
        torch.cuda.synchronize()
    run_order([3, 0, 5, 2, 1, 6, 4, 7, 0], before_each)
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'
    eng = shared()[1].engine()
    assert eng._ws_bop and 'SamplingEngine._ws_bop' in co.kept_tensors(*shared())
