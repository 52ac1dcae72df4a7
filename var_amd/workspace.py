"""The buffer sets of SamplingEngine: what is in one, as a table computed from shapes alone, the allocator that turns the
table into tensors, and the one rule by which the engine's caches hold, replace and drop such sets.  Nothing here launches a kernel."""
from typing import Callable, Dict, NamedTuple, Optional

import torch


class Dims(NamedTuple):
    """what a buffer set takes from the model"""
    C: int                  # embedding width
    H: int                  # heads (of 64 channels each)
    V: int                  # vocabulary
    Cvae: int               # channels of a code
    P: int                  # side of the last scale's map
    depth: int              # blocks
    hidden: int             # width of a block's MLP
    shared_aln: bool
    L: int                  # tokens of all scales


PER_BLOCK = ('kc', 'vc')    # entries whose shape leads with `depth`: allocate() makes them a list of one tensor per block


def sampler_rows(d: Dims, B: int, lmax: int) -> dict:
    """the sampler's own rows, one per token of B images at the widest scale, which SamplingEngine._masked adds to a set on first use: the
    filtered logits, and for more_smooth the gumbel-softmax probabilities and their embedding"""
    f32 = torch.float32
    return {'masked': ((B * lmax, d.V), f32, False), 'probs': ((B * lmax, d.V), f32, False), 'h': ((B * lmax, d.Cvae), f32, False)}


def workspace_spec(d: Dims, act: torch.dtype, R: int, lmax: int, Lkv: int, *, B: int = 0, twin: bool = False, logits: str = 'logits',
                   masked: bool = False, mixed: bool = False, Lmax: bool = False) -> Dict[str, Optional[tuple]]:
    """{name: (shape, dtype, zeroed)} of the buffer set of a pass of R transformer rows whose widest scale has lmax tokens, over KV caches of
    Lkv tokens.  act: the type of the GEMM operands and the caches (the residual stream, the AdaLN tables and the logits are fp32).  Two
    entries are no such triple and allocate() hands them on as they are: `shared` is None without shared_aln, `Lmax` is the int Lkv.
    On top of the transformer's buffers:
      B       the quantizer step's buffers for B images (idx, f_hat, up, pooled)
      twin    the prologue is handed all R rows as labels (a composed or a teacher-forced pass; a plain sampling call hands it B labels for its
              R = 2B rows).  first_map_f32 writes behind the R conditions and first maps it is asked for the unconditional twin of each, and
              word_embed_f32 behind the R * l rows of a scale's input their CFG copies: cond, cond_silu and x have room for 2x
      logits  the name of the head's output ('lg' in a teacher-forced set)
      masked  the filtered rows of B images (sampler_rows)
      mixed   the guided rows of a composed pass, followed by as many zero rows: varhip_sample_stats_f32 reads the 2 * B * lmax rows as CFG
              pairs with t = 0
      Lmax    the set records its cache length for block()"""
    f32 = torch.float32
    M, t = R * lmax, 2 if twin else 1
    s = {'x': ((t * M, d.C), f32, False), 'x2': ((M, d.C), f32, False), 'xn': ((M, d.C), act, False), 'q': ((M, d.C), act, False),
         'att': ((M, d.C), act, False), 'hid': ((M, d.hidden), act, False), logits: ((M, d.V), f32, False)}
    if B:
        s['idx'] = ((B * lmax,), torch.int64, False)
    s.update({
        'lvl_pos': ((d.L, d.C), f32, False), 'cond': ((t * R, d.C), f32, False), 'cond_silu': ((t * R, d.C), f32, False),
        'hn': ((R, 2 * d.C), f32, False),       # AdaLNBeforeHead's scale | shift of every row: ln_modulate reads hn and hn[:, C:] at stride 2C
        'ada': ((d.depth, R, 6 * d.C) if d.shared_aln else (R, d.depth * 6 * d.C), f32, False),
        'shared': ((R, 6 * d.C), f32, False) if d.shared_aln else None,
        'kc': ((d.depth, R, d.H, Lkv, 64), act, True), 'vc': ((d.depth, R, d.H, Lkv, 64), act, True)})
    if B:
        s.update({'f_hat': ((B, d.P, d.P, d.Cvae), f32, False), 'up': ((B, d.P, d.P, d.Cvae), f32, False), 'pooled': ((B * lmax, d.Cvae), f32, False)})
    if masked:
        s['masked'] = sampler_rows(d, B, lmax)['masked']
    if mixed:
        s['mixed'] = ((2 * B * lmax, d.V), f32, False)
    if Lmax:
        s['Lmax'] = Lkv
    return s


def allocate(spec: dict, dev) -> dict:
    """the buffer set of a spec on `dev`: {'dev': dev, name: tensor}, the PER_BLOCK entries lists of one tensor per block"""
    make = lambda shape, dt, zeroed: (torch.zeros if zeroed else torch.empty)(shape, dtype=dt, device=dev)
    ws = {'dev': dev}
    for name, v in spec.items():
        if not isinstance(v, tuple):
            ws[name] = v
        elif name in PER_BLOCK:
            ws[name] = [make(v[0][1:], *v[1:]) for _ in range(v[0][0])]
        else:
            ws[name] = make(*v)
    return ws


def cached(cache: dict, size: int, slot: tuple, bound: int, dev, alloc: Callable[[], dict]) -> dict:
    """the buffer set cache[(size, *slot)], slot = (HIP stream, precision, ...), made by alloc() unless the cache holds it on `dev`.  One size
    is resident per slot and at most `bound` sets per cache: the slot's other sizes go, then the oldest sets of other slots, and only then
    alloc() runs, so the replaced set is free before the new one is allocated (a d16 / B=64 set is 6-11 GB; its memory returns to the stream
    it was allocated on, so work still queued there is safe)"""
    key = (size,) + slot
    ws = cache.get(key)
    if ws is None or ws['dev'] != dev:
        ws = None
        for k in [k for k in cache if k[1:] == slot]:
            del cache[k]
        while len(cache) >= bound:
            del cache[next(iter(cache))]
        ws = cache[key] = alloc()
    return ws


def keep_precision(cache: dict, precision: str):
    """drop the sets of every other precision (the second element of a slot)"""
    for k in [k for k in cache if k[2] != precision]:
        del cache[k]
