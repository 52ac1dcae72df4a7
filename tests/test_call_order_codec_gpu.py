"""Call-order independence of VAR.compress / VAR.decompress (tests/test_call_order_gpu.py has the method): interleaved with sampling, SMC, the
scorer and a precision switch there and back, in three orders and once more with every workspace poisoned, a call's blobs and tokens are the
bytes it gives as the first call on a fresh model."""
import collections

import numpy as np
import pytest
import torch

from tests import test_call_order_gpu as co
from tests import test_call_order_smc_gpu as smc

pytestmark = pytest.mark.gpu

Entry = collections.namedtuple('Entry', 'name policy autocast fn raises')
_ALONE, _SHARED = {}, {}


def _tokens():
    gt = co.scoring_gt()                                     # two images of the fixture, and one of uniform random tokens (a long stream)
    rnd = torch.randint(0, 4096, (1, gt.shape[1]), generator=torch.Generator().manual_seed(9)).cuda()
    return torch.cat((gt[:2], rnd)), torch.tensor(co.labels_of(3), device='cuda')


def _blob_tensors(blobs):
    return {f'blob{i}': torch.from_numpy(np.frombuffer(b, np.uint8).copy()) for i, b in enumerate(blobs)}


def compress(cfg, scales=None):
    def fn(vae, var):
        tok, lab = _tokens()
        r = var.compress(tok, lab, cfg=cfg, scales=scales)
        return dict(nbytes=r.nbytes, ideal=r.ideal_bits, **_blob_tensors(r.blobs))
    return fn


def round_trip(complete):
    def fn(vae, var):
        tok, lab = _tokens()
        r = var.compress(tok, lab, cfg=1.5, scales=None if complete is None else 2)
        out = var.decompress(r.blobs[::-1], complete=complete)
        return dict(tokens=out.tokens, img=out.images, labels=out.labels, **_blob_tensors(r.blobs))
    return fn


def bad_precision(vae, var):
    tok, lab = _tokens()
    var.compress(tok, lab)


DECK = [Entry('compress', 'f32', False, compress(1.5), None), Entry('ar', 'f32', False, co.ar(2, 5), None),
        Entry('round trip', 'f32', False, round_trip(None), None), Entry('smc bf16', 'bf16', False, smc.smc, None),
        Entry('compress cfg 0', 'f32', False, compress(0.0), None), Entry('loglik', 'f32', False, co.loglik, None),
        Entry('compress refused in f16', 'f16', False, bad_precision, ValueError), Entry('round trip greedy', 'f32', False, round_trip('greedy'), None),
        Entry('smc f32', 'f32', False, smc.smc, None)]
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


def test_the_alone_round_trip_returns_its_tokens():
    """the call the other tests compare: it must decode what it coded, or the orders below show nothing"""
    tok, _ = _tokens()
    assert torch.equal(alone(DECK[2])['tokens'], tok.flip(0).cpu())


@pytest.mark.parametrize('order', [list(range(N)), list(reversed(range(N))), [7, 0, 3, 2, 5, 6, 4, 1, 8, 0, 2]], ids=['listed', 'reverse', 'mixed'])
def test_every_order_gives_the_alone_results(order):
    run_order(order)


def test_poisoned_workspaces_change_nothing(monkeypatch):
    monkeypatch.setattr(co, 'POISONED', co.POISONED | {'SamplingEngine._ws_bop'})
    run_order(list(range(N)))                                # (run on its own: give the model a history first)
    written = []

    def before_each():
        torch.cuda.synchronize()
        written.append(co.poison_engines(*shared()))
        co.poison_allocator()
        torch.cuda.synchronize()
    run_order([7, 0, 3, 2, 5, 6, 4, 1, 8, 0, 2], before_each)
    assert max(written) >= 20, 'the poisoned pass found no workspace to poison'
