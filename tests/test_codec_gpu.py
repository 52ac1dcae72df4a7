"""VAR.compress / VAR.decompress on the GPU: round trips, independence of batch and order, the walk's tables against the scorer's numbers, the
size of a blob, partial coding with greedy completion, every refusal, and that a call keeps no state."""
import math

import pytest
import torch

from tests.test_best_of_pruned_gpu import _model
from var_amd import abi
from var_amd.models.var import VarCodecError, codec_unpack

pytestmark = pytest.mark.gpu

PB = abi.CODEC_PB
_TOK = {}


def tokens_of(name):
    """(var, labels (3,), tokens (3, L)): two images sampled by the model (likely under it: short streams), one of uniform random tokens
    (unlikely: about 12 bits per token at V = 4096); computed once and left unchanged"""
    var, lab2 = _model(name)
    if name not in _TOK:
        lab = torch.cat((lab2, torch.tensor([var.num_classes], device='cuda')))             # the unconditional class is a legal label
        _, tok = var.autoregressive_infer_cfg_per_image(lab2, [5, 6], cfg=1.5, top_k=900, top_p=0.96, return_tokens=True)
        rnd = torch.randint(0, var.V, (1, var.L), generator=torch.Generator().manual_seed(3)).cuda()
        _TOK[name] = (lab, torch.cat((tok, rnd)))
    return (var,) + _TOK[name]


def header_bits(var):
    return 8 * (44 + 2 * len(var.patch_nums))


@pytest.mark.parametrize('name', ['t_pn12345', 'd16_pn123'])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_round_trip_tokens_images_and_size(name, cfg):
    var, lab, tok = tokens_of(name)
    res = var.compress(tok, lab, cfg=cfg)
    out = var.decompress(res.blobs)
    assert torch.equal(out.tokens, tok) and torch.equal(out.labels, lab) and out.scales == len(var.patch_nums) - 1
    # the existing route from tokens to pixels on the same walk: inpainting with every token kept
    want = var.inpainting(tok, torch.ones_like(tok, dtype=torch.bool), label=lab, cfg=cfg)
    assert torch.equal(out.images.view(torch.int32), want.view(torch.int32))
    assert var.decompress(res.blobs, decode=False).images is None
    assert res.nbytes.tolist() == [len(b) for b in res.blobs] and tuple(res.ideal_bits.shape) == (3, len(var.patch_nums))
    bound = header_bits(var) + res.ideal_bits.sum(1) + var.L / 64 + 64
    print(name, cfg, 'bytes', res.nbytes.tolist(), 'ideal bits', res.ideal_bits.sum(1).tolist())
    assert (res.nbytes * 8 <= bound).all(), (res.nbytes * 8, bound)
    assert torch.equal(var.compress(list(tok[:, b:e] for b, e in var.begin_ends), lab, cfg=cfg).nbytes, res.nbytes)      # the list form


def test_blobs_do_not_depend_on_batch_or_order():
    var, lab, tok = tokens_of('t_pn12345')
    res = var.compress(tok, lab, cfg=1.5)
    for b in range(3):                                                  # compressed one at a time: byte-identical
        assert var.compress(tok[b:b + 1], lab[b:b + 1], cfg=1.5).blobs[0] == res.blobs[b], b
    assert var.compress(tok.flip(0), lab.flip(0), cfg=1.5).blobs == res.blobs[::-1]
    for b in range(3):                                                  # decoded one at a time
        assert torch.equal(var.decompress(res.blobs[b:b + 1], decode=False).tokens, tok[b:b + 1]), b
    assert torch.equal(var.decompress(res.blobs[::-1], decode=False).tokens, tok.flip(0))
    other = var.compress(tok[:1], torch.tensor([17], device='cuda'), cfg=1.5)               # the same tokens under another label
    assert other.blobs[0] != res.blobs[0]
    mix = var.decompress([res.blobs[2], other.blobs[0], res.blobs[0], res.blobs[1]], decode=False)
    assert torch.equal(mix.tokens, tok[[2, 0, 0, 1]]) and mix.labels.tolist() == [int(lab[2]), 17, int(lab[0]), int(lab[1])]


@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_ideal_bits_against_the_scorer(cfg):
    """ideal_bits.sum() <= B1 + s, B1 = sum min(24, -log2(p (1 - 2^-11) - 2^-24)) (24 where the argument is not positive) over the tokens with
    p = exp(lp), lp = token_log_likelihood's fp32 value: the table's own guarantee F / 2^24 >= p64 (1 - 2^-11) - 2^-24 holds for
    the float64 softmax p64 of the row, and every F >= 1 caps a token at 24 bits.
    The slack s turns the scorer's bar |lp - lp64| <= d, d = 1e-6 (|lp64| + max|z| + 8) (tests/test_likelihood_gpu.py::kernel_bar_ok), into
    bits.  g(p) = min(24, -log2(p (1 - e) - h)), e = 2^-11, h = 2^-24, falls in p, and where it is below 24, p (1 - e) - h >= 2^-24 = h, so
    |dg / d ln p| = (1 / ln 2) p (1 - e) / (p (1 - e) - h) <= 2 / ln 2.  With p64 >= p exp(-d): g(p64) <= g(p) + 2 d / ln 2 per token, and
    s = sum 2 d / ln 2."""
    from tests.test_likelihood_gpu import kernel_bar_ok
    var, lab, tok = tokens_of('t_pn12345')
    S = len(var.patch_nums)
    res = var.compress(tok, lab, cfg=cfg)
    lp = var.token_log_likelihood(tok, lab.view(-1, 1), cfg=cfg)[:, 0].double()             # (3, L)
    with torch.no_grad():
        x = var.vae_proxy[0].quantize.idxBl_to_var_input([tok[:, b:e] for b, e in var.begin_ends])
        cond = var.engine().teacher_forced_logits(lab, x).double()
        unc = var.engine().teacher_forced_logits(torch.full_like(lab, var.num_classes), x).double()
    t = torch.tensor([cfg * si / (S - 1) for si, pn in enumerate(var.patch_nums) for _ in range(pn * pn)], device='cuda', dtype=torch.float64).view(1, -1, 1)
    z = (1 + t) * cond - t * unc
    lp64 = torch.log_softmax(z, -1).gather(-1, tok.unsqueeze(-1))[..., 0]
    ok, worst = kernel_bar_ok(lp.float(), lp64, z.float())
    assert ok, worst                                                    # the bar the slack is made of holds here
    d = 1e-6 * (lp64.abs() + z.abs().amax(-1) + 8)
    s = float((2 * d / math.log(2)).sum())
    arg = lp.exp() * (1 - 2.0 ** -11) - 2.0 ** -PB
    per = torch.where(arg > 0, -torch.log2(arg.clamp_min(1e-300)), torch.full_like(arg, float(PB))).clamp_max(float(PB))
    B1 = float(per.sum())
    ideal = float(res.ideal_bits.sum())
    nats = float(-lp.sum() / math.log(2))
    print(f'cfg={cfg}: ideal_bits {ideal:.3f}, -sum lp / ln 2 {nats:.3f} (difference {ideal - nats:+.3f}), B1 {B1:.3f}, slack {s:.4f}')
    assert ideal <= B1 + s, (ideal, B1, s)


def test_partial_coding_and_greedy_completion():
    var, lab, tok = tokens_of('t_pn12345')
    n = var.begin_ends[2][1]
    res = var.compress(tok, lab, cfg=1.5, scales=2)
    assert all(codec_unpack(b)['coded'] == 3 for b in res.blobs) and bool((res.ideal_bits[:, 3:] == 0).all())
    out = var.decompress(res.blobs, complete=None)
    assert out.scales == 2 and torch.equal(out.tokens[:, :n], tok[:, :n]) and bool((out.tokens[:, n:] == -1).all()) and out.images is not None
    fill = var.decompress(res.blobs, complete='greedy', fill_cfg=1.5)
    assert torch.equal(fill.tokens[:, :n], tok[:, :n]) and int(fill.tokens.min()) >= 0
    keep = torch.zeros_like(tok, dtype=torch.bool)
    keep[:, :n] = True
    want_tok = torch.empty_like(tok)
    want = var.engine().sample(3, lab, None, 1.5, 0, 0.0, gt_tokens=tok, keep_mask=keep, greedy=True, tokens_out=want_tok)      # classify_generative's route
    assert torch.equal(fill.tokens, want_tok) and torch.equal(fill.images.view(torch.int32), want.view(torch.int32))
    assert res.nbytes.max() < 44 + 2 * 5 + 4 * (n + 2) + 1


def test_refusals():
    var, lab, tok = tokens_of('t_pn12345')
    res = var.compress(tok, lab, cfg=1.5)
    try:
        for prec in ('f16', 'bf16'):
            var.set_hip_precision(prec)
            with pytest.raises(ValueError, match='f32'):
                var.compress(tok, lab)
            with pytest.raises(ValueError, match='f32'):
                var.decompress(res.blobs)
        var.set_hip_precision('auto')
        with torch.autocast('cuda', dtype=torch.float16), pytest.raises(ValueError, match='f32'):
            var.decompress(res.blobs)
        assert torch.equal(var.decompress(res.blobs, decode=False).tokens, tok)             # 'auto' outside an autocast region is f32
    finally:
        var.set_hip_precision('f32')
    with pytest.raises(ValueError, match='cfg'):
        var.decompress([res.blobs[0], var.compress(tok[1:2], lab[1:2], cfg=0.5).blobs[0]])
    with pytest.raises(ValueError, match='coded scales'):
        var.decompress([res.blobs[0], var.compress(tok[1:2], lab[1:2], cfg=1.5, scales=1).blobs[0]])
    small, lab_s, tok_s = tokens_of('d16_pn123')
    with pytest.raises(ValueError, match='patch_nums'):
        var.decompress(small.compress(tok_s, lab_s).blobs)
    for bad in (b'', res.blobs[0][:-1], b'XXXX' + res.blobs[0][4:], 7):
        with pytest.raises(ValueError):
            var.decompress([bad])
    with pytest.raises(ValueError):
        var.compress(tok[:, :-1], lab)
    with pytest.raises(ValueError):
        var.compress(tok, lab[:2])
    with pytest.raises(ValueError):
        var.compress(tok, lab, scales=5)
    head = 44 + 2 * len(var.patch_nums)
    flipped = bytearray(res.blobs[1]); flipped[head + 4 * 3 + 1] ^= 0x10
    with pytest.raises(VarCodecError, match='image 1') as ei:
        var.decompress([res.blobs[0], bytes(flipped), res.blobs[2]])
    assert ei.value.image == 1 and ei.value.check in ('bounds', 'end', 'hash')
    wrong_hash = bytearray(res.blobs[2]); wrong_hash[32] ^= 1
    with pytest.raises(VarCodecError, match='image 2') as ei:
        var.decompress([res.blobs[0], res.blobs[1], bytes(wrong_hash)])
    assert ei.value.check == 'hash'


def test_other_weights_and_cpu_model():
    var, lab, tok = tokens_of('t_pn12345')
    blobs = var.compress(tok, lab, cfg=1.5).blobs
    from tests import test_e2e_gpu
    cached = dict(test_e2e_gpu._MODELS)
    other, _ = _model('t_pn12345', fresh=True)                          # a model of its own; the cached ones are put back below
    try:
        assert other is not var
        assert torch.equal(other.decompress(blobs, decode=False).tokens, tok)               # the same weights in another object: the same tables
        torch.manual_seed(1234)
        other.init_weights(init_adaln=0.5, init_adaln_gamma=1e-5, init_head=0.02, init_std=0.02)
        with pytest.raises(VarCodecError, match='image 0'):
            other.decompress(blobs, decode=False)
        cpu = other.cpu()
        with pytest.raises(RuntimeError, match='HIP'):
            cpu.compress(tok.cpu(), lab.cpu())
        with pytest.raises(RuntimeError, match='HIP'):
            cpu.decompress(blobs)
    finally:
        test_e2e_gpu._MODELS.clear()
        test_e2e_gpu._MODELS.update(cached)


def test_the_call_keeps_no_state():
    var, lab, tok = tokens_of('t_pn12345')
    res = var.compress(tok, lab, cfg=1.5)
    var.decompress(res.blobs)                                           # (both calls have run once: their workspace exists)
    rng = var.rng.get_state().clone()
    nws = len(var.engine()._ws)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    res2 = var.compress(tok, lab, cfg=1.5)
    out = var.decompress(res2.blobs)
    assert res2.blobs == res.blobs and torch.equal(out.tokens, tok)
    del out, res2
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before and len(var.engine()._ws) == nws
    assert torch.equal(var.rng.get_state(), rng)
