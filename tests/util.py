"""Shared helpers of the test-suite: deterministic weights, golden loading, noise regeneration, comparison reports."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from var_amd import shapes                          # noqa: E402
from var_amd.detinit import make_state_dict         # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
_WCACHE = {}


def ensure_oracle_built():
    so = os.path.join(ROOT, 'oracle', 'libvar_oracle.so')
    src = os.path.join(ROOT, 'oracle', 'var_oracle.c')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(['make', '-C', os.path.join(ROOT, 'oracle')], stdout=subprocess.DEVNULL)


def load_case(name):
    z = np.load(os.path.join(GOLD, f'e2e_{name}.npz'))
    meta = json.loads(str(z['meta']))
    return z, meta


def make_weights(meta, seed=0, include_encoder=False):
    """Deterministic VAR + VQVAE weights in the reference's state-dict layout (numpy), cached per config."""
    key = (meta['depth'], meta['ch'], tuple(meta['patch_nums']), meta['attn_l2_norm'], meta['shared_aln'], seed, include_encoder)
    if key in _WCACHE:
        return _WCACHE[key]
    pns = tuple(meta['patch_nums'])
    vs = shapes.var_shapes(meta['depth'], pns, shared_aln=meta['shared_aln'], attn_l2_norm=meta['attn_l2_norm'])
    var_sd = make_state_dict(vs, depth=meta['depth'], seed=seed, prefix='var.')
    var_sd['lvl_1L'] = np.concatenate([np.full((p * p,), i, dtype=np.int64) for i, p in enumerate(pns)]).reshape(1, -1)
    es = shapes.vae_shapes(ch=meta['ch'], patch_nums=pns, include_encoder=include_encoder)
    vae_sd = make_state_dict(es, depth=meta['depth'], seed=seed, prefix='vae.')
    _WCACHE.clear()          # keep at most one config resident (d16 is 1.6 GB)
    _WCACHE[key] = (var_sd, vae_sd)
    return var_sd, vae_sd


def regen_noise(meta, z=None):
    """The Exp(1) fills torch.multinomial(n=1) consumed in the reference run, one (B*l, V) fill per scale, regenerated
    with a CPU torch.Generator (same wheel on both boxes) and checked against the fixture's head/checksum."""
    import torch
    g = torch.Generator(device='cpu')
    g.manual_seed(meta['seed'])
    out = []
    for si, pn in enumerate(meta['patch_nums']):
        q = torch.empty(meta['B'] * pn * pn, meta['V'], dtype=torch.float32).exponential_(1, generator=g)
        if z is not None:
            assert np.array_equal(q.view(-1)[:8].numpy(), z['noise_head'][si]), 'torch CPU RNG stream differs from the fixture'
            assert abs(q.double().sum().item() - float(z['noise_sum'][si])) <= 1e-6 * abs(float(z['noise_sum'][si]))
        out.append(q.numpy())
    return out


def diff_report(name, got, want, atol=0.0, rtol=0.0):
    """Returns (ok, message) with max abs error, mismatch count and first mismatch index."""
    got = np.asarray(got); want = np.asarray(want)
    if got.shape != want.shape:
        return False, f'{name}: shape {got.shape} != {want.shape}'
    if got.dtype.kind in 'iub':
        bad = got != want
        nbad = int(bad.sum())
        return nbad == 0, f'{name}: {nbad}/{got.size} mismatches' + (f', first at {tuple(np.argwhere(bad)[0])}' if nbad else '')
    g64, w64 = got.astype(np.float64), want.astype(np.float64)
    with np.errstate(invalid='ignore'):
        close = np.abs(g64 - w64) <= atol + rtol * np.abs(w64)
    bad = ~(close | (got == want) | (np.isnan(got) & np.isnan(want)))
    nbad = int(bad.sum())
    d = np.abs(g64 - w64)
    fin = np.isfinite(d)
    mx = float(d[fin].max()) if fin.any() else 0.0
    wfin = np.isfinite(w64)
    msg = f'{name}: max|d|={mx:.3e} (|want| max {float(np.abs(w64[wfin]).max()) if wfin.any() else 0:.3e}), {nbad}/{got.size} outside atol={atol:g} rtol={rtol:g}'
    if nbad:
        i = tuple(np.argwhere(bad)[0]); msg += f', first at {i}: got {got[i]!r} want {want[i]!r}'
    return nbad == 0, msg


def free_port() -> int:
    """a TCP port nobody listens on right now (rendezvous of child process groups on 127.0.0.1)"""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


# ---------------------------------------------------------------------------------------------------------------------
# Guard bands ("memory contract of the ABI").  An arena is one uint8 allocation laid out as  band | operand bytes | band  with
# both bands filled with 0xFF: a NaN in fp16 / bf16 / fp32 / fp64, -1 in int32 / int64, 255 in uint8.  A float read from a band poisons the
# result, an index read from a band is -1 and points into the band in front of whatever it indexes, and a store into a band is found after
# the call.  One code path serves numpy arrays (host: the oracle's twins) and torch tensors (device: the HIP kernels).
GUARD_BYTE = 0xFF
GUARD_MIN, GUARD_CAP, GUARD_ALIGN = 4096, 1 << 20, 512


class GuardError(AssertionError):
    """a band changed; .findings = [dict(name, args, band ('front' | 'back'), first, last, nbytes)], offsets in bytes relative to the operand's first byte"""
    def __init__(self, msg, findings):
        super().__init__(msg)
        self.findings = findings


def guard_band_bytes(nbytes):
    """band length for an operand of nbytes: its own length, at least 4 KiB, at most 1 MiB (the largest window a buffer descriptor in the
    tree declares in front of its operand is 164 KB), rounded up to 512 B so that the operand keeps the allocator's alignment"""
    n = min(max(int(nbytes), GUARD_MIN), GUARD_CAP)
    return (n + GUARD_ALIGN - 1) // GUARD_ALIGN * GUARD_ALIGN


def _is_torch(x):
    return hasattr(x, 'data_ptr') and hasattr(x, 'storage_offset')


def _addr(x):
    return int(x.data_ptr()) if _is_torch(x) else int(x.ctypes.data)


def _span_bytes(x):
    """the storage a view addresses, from its first to its last element, as a flat writable uint8 view of the caller's own memory
    (None: the view has no element)"""
    if _is_torch(x):
        import torch
        if x.numel() == 0:
            return None
        assert all(s >= 0 for s in x.stride()), 'guard bands: negative strides are not supported'
        n = 1 + sum((d - 1) * s for d, s in zip(x.shape, x.stride()))
        return x.as_strided((n,), (1,), x.storage_offset()).view(torch.uint8)
    import ctypes
    if x.size == 0:
        return None
    assert all(s >= 0 for s in x.strides), 'guard bands: negative strides are not supported'
    n = x.itemsize + sum((d - 1) * s for d, s in zip(x.shape, x.strides))
    return np.frombuffer((ctypes.c_uint8 * n).from_address(x.ctypes.data), dtype=np.uint8)


def _changed(v):
    """(first, last) index of the bytes of band v that are no longer 0xFF, or None"""
    bad = v != GUARD_BYTE
    if not bool(bad.any()):
        return None
    idx = np.flatnonzero(bad) if isinstance(bad, np.ndarray) else bad.nonzero().flatten()
    return int(idx[0]), int(idx[-1])


class GuardArena:
    """band | operand bytes | band for the bytes [addr, addr + nbytes) of the caller's memory; `like` decides host or device.
    The operand keeps its address modulo 512 B (an interior pointer stays as misaligned as it was)."""
    def __init__(self, like, addr, nbytes, positions):
        self.addr, self.nbytes, self.positions = addr, nbytes, positions
        self.band = guard_band_bytes(nbytes)
        total = GUARD_ALIGN + self.band + GUARD_ALIGN + nbytes + self.band
        if _is_torch(like):
            import torch
            self.buf = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=like.device)
        else:
            self.buf = np.full(total, GUARD_BYTE, np.uint8)
        self.base = _addr(self.buf)
        self.o0 = (-self.base) % GUARD_ALIGN + self.band + addr % GUARD_ALIGN          # the front band is at least `band` long

    def _slice(self, addr, n):
        d = self.o0 + addr - self.addr
        assert self.o0 <= d and d + n <= self.o0 + self.nbytes
        return slice(d, d + n)

    def put(self, addr, b):
        self.buf[self._slice(addr, len(b))] = b

    def get(self, addr, b):
        b[:] = self.buf[self._slice(addr, len(b))]

    def ptr(self, addr):
        return self.base + self.o0 + addr - self.addr

    def findings(self, name):
        out = []
        for band, v, rel in (('front', self.buf[:self.o0], -self.o0), ('back', self.buf[self.o0 + self.nbytes:], self.nbytes)):
            c = _changed(v)
            if c is not None:
                out.append(dict(name=name, args=list(self.positions), band=band, first=c[0] + rel, last=c[1] + rel, nbytes=self.nbytes))
        return out


def guard_layout(args):
    """-> (arenas, [(position, address, span bytes, arena)]) for the array arguments of `args`; operands that overlap in storage (the same
    tensor passed twice, two views of one buffer, an in-place x) share one arena"""
    spans = []
    for pos, a in enumerate(args):
        if isinstance(a, np.ndarray) or _is_torch(a):
            b = _span_bytes(a)
            if b is not None:
                space = str(a.device) if _is_torch(a) else 'host'
                spans.append((space, _addr(a), pos, b, a))
    spans.sort(key=lambda s: (s[0], s[1], s[2]))
    groups = []
    for space, addr, pos, b, a in spans:
        g = groups[-1] if groups else None
        if g is not None and g['space'] == space and addr < g['end']:
            g['end'] = max(g['end'], addr + len(b)); g['members'].append((pos, addr, b))
        else:
            groups.append(dict(space=space, addr=addr, end=addr + len(b), like=a, members=[(pos, addr, b)]))
    arenas, placed = [], []
    for g in groups:
        ar = GuardArena(g['like'], g['addr'], g['end'] - g['addr'], sorted(m[0] for m in g['members']))
        for pos, addr, b in g['members']:
            ar.put(addr, b)
            placed.append((pos, addr, b, ar))
        arenas.append(ar)
    return arenas, placed


def guarded_invoke(name, args, invoke, sync=None):
    """invoke(*args) with every array argument replaced by a pointer to its copy inside a guard arena; afterwards every band must still be
    all 0xFF (GuardError names the entry point, the argument, the band and the changed byte range), and the operand bytes are copied back
    into the caller's arrays.  Returns what invoke returned."""
    import ctypes
    arenas, placed = guard_layout(args)
    new = list(args)
    for pos, a in enumerate(args):
        if isinstance(a, np.ndarray) or _is_torch(a):
            new[pos] = ctypes.c_void_p(_addr(a))                   # (an array without elements: its own pointer)
    for pos, addr, b, ar in placed:
        new[pos] = ctypes.c_void_p(ar.ptr(addr))
    rc = invoke(*new)
    if sync is not None:
        sync()
    found = [f for ar in arenas for f in ar.findings(name)]
    if found:
        raise GuardError('; '.join(
            f"{f['name']}: argument {', '.join(map(str, f['args']))}{' (one shared arena)' if len(f['args']) > 1 else ''}: the band "
            f"{'in front of' if f['band'] == 'front' else 'behind'} the operand was written, bytes {f['first']} to {f['last']} relative to "
            f"the operand's first byte (operand: {f['nbytes']} bytes)" for f in found), found)
    for pos, addr, b, ar in placed:
        ar.get(addr, b)
    return rc


def guarded_call(name, *args, stream=None):
    """drop-in for var_amd.hip.call in tests: every tensor argument lives in a guard arena during the call"""
    import torch
    from var_amd import hip
    if stream is not None:
        torch.cuda.synchronize()
    return guarded_invoke(f'varhip_{name}', args, lambda *a: hip.call(name, *a, stream=stream), torch.cuda.synchronize)
