"""Device side of tests/test_gpu_seq.py: one call of clv_lstm_seq_fwd / _bwd / _bwd_z on buffers that show a stray access --
every output a helpers.Bufs buffer (NaN inside, a canary tail, the canary in the lddz padding), every input in the middle of
a NaN-filled buffer, so a read outside it that reaches an output shows -- run twice and compared bit for bit.

As a program (python tests/seq_worker.py OUT.npz) it runs the lstm.hip forward table and the 88-unit impulse probes of
tests/seq_reference.py and writes inputs and outputs to OUT.npz; tests/test_gpu_seq.py starts it as a fresh child process with
CLV_LSTM_KS=8 in its environment (the knob is read once per process) and judges what it wrote."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import seq_reference as S  # noqa: E402
from helpers import Bufs  # noqa: E402

PAD = 64                    # NaN floats in front of and behind every input


class Base:
    """stands in for a tensor without elements (T = 0): torch reports NULL as the address of an empty tensor, the entry points
    want the buffer's"""

    def __init__(self, t, raw):
        self.t, self.raw = t, raw

    def data_ptr(self):
        return self.raw.data_ptr()


def N(t):
    return (t.t if isinstance(t, Base) else t).detach().cpu().numpy()


def based(bufs, t):
    """t, a buffer that bufs handed out last"""
    return t if t.numel() else Base(t, bufs.all[-1][0])


def nan_wrap(torch, dev, a):
    """a on the device with PAD NaN floats on either side"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32)
    full = np.full(a.size + 2 * PAD, np.nan, np.float32)
    full[PAD:PAD + a.size] = a.ravel()
    raw = torch.as_tensor(full, device=dev)
    t = raw[PAD:PAD + a.size].view(*a.shape)
    return t if a.size else Base(t, raw[PAD:])


class forced_any:
    """CLV_LSTM_ANY=1 around a call (the library reads it per call): 88 units through csrc/lstm_any.hip"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("CLV_LSTM_ANY")
        if self.on:
            os.environ["CLV_LSTM_ANY"] = "1"

    def __exit__(self, *exc):
        if self.on:
            if self.old is None:
                del os.environ["CLV_LSTM_ANY"]
            else:
                os.environ["CLV_LSTM_ANY"] = self.old


def forward_once(torch, dev, c, inp, state_inplace=False):
    """one clv_lstm_seq_fwd call of case c -> {output: array}; state_inplace: hT / cT are the buffers of h0 / c0"""
    from clvae_amd import ops
    x = inp['xproj']
    B, T, H = x.shape[0], x.shape[1], x.shape[2] // 4
    save = bool(c.get('save', 1)) and not state_inplace
    own = bool(c.get('own', 0)) or not save
    bufs = Bufs(dev)
    xp = nan_wrap(torch, dev, x) if own else based(bufs, bufs.inp(x))
    gates = (based(bufs, bufs.out(B, T, 4 * H)) if own else xp) if save else None
    cs = based(bufs, bufs.out(B, T, H)) if save else None
    hs = based(bufs, bufs.out(B, T, H))
    alias = bool(c.get('alias', 0)) or state_inplace
    h0 = None if inp['h0'] is None else bufs.inp(inp['h0']) if alias else nan_wrap(torch, dev, inp['h0'])
    c0 = None if inp['c0'] is None else bufs.inp(inp['c0']) if state_inplace else nan_wrap(torch, dev, inp['c0'])
    hT = None if not c.get('hT', 1) else h0 if alias and h0 is not None else bufs.out(B, H)
    cT = None if not c.get('cT', 1) else c0 if state_inplace and c0 is not None else bufs.out(B, H)
    with forced_any(c.get('force', 0)):
        ops.lstm_seq_fwd(B, T, xp, nan_wrap(torch, dev, inp['rowbias']), nan_wrap(torch, dev, inp['U']), hs, cs, gates,
                         h0=h0, c0=c0, hT=hT, cT=cT, gate_act=inp['gate_act'], H=H)
    torch.cuda.synchronize()
    bufs.check_canaries()
    got = dict(hs=N(hs))
    if save:
        got.update(cs=N(cs), gates=N(gates))
        if own:
            got['xproj_after'] = N(xp)
    if hT is not None:
        got['hT'] = N(hT)
    if cT is not None:
        got['cT'] = N(cT)
    return got


def backward_once(torch, dev, rec, dhs, Uw, c0, gate_act, Kz=None, pad=0, force=0):
    """one clv_lstm_seq_bwd (Kz None) or clv_lstm_seq_bwd_z call on the records -> dz, dzsum, dZ [B,T,nz]"""
    from clvae_amd import ops
    B, T, H = rec['cs'].shape
    bufs = Bufs(dev)
    gates = based(bufs, bufs.inp(rec['gates']))
    dzsum = bufs.out(B, 4 * H)
    args = (B, T, nan_wrap(torch, dev, Uw), nan_wrap(torch, dev, dhs), nan_wrap(torch, dev, rec['cs']), gates, dzsum)
    kw = dict(c0=nan_wrap(torch, dev, c0), gate_act=gate_act, H=H)
    with forced_any(force):
        if Kz is None:
            ops.lstm_seq_bwd(*args, **kw)
        else:
            nz = Kz.shape[0]
            dZ = based(bufs, bufs.out(B * T, nz + pad, pad_cols=pad))
            ops.lstm_seq_bwd_z(*args, nan_wrap(torch, dev, Kz), nz, dZ, nz + pad, **kw)
    torch.cuda.synchronize()
    bufs.check_canaries()
    got = dict(dz=N(gates), dzsum=N(dzsum))
    if Kz is not None:
        got['dZ'] = np.ascontiguousarray(N(dZ)[:, :Kz.shape[0]]).reshape(B, T, Kz.shape[0])
    return got


def twice(name, fn):
    """fn() two times; the two results bit for bit"""
    a, b = fn(), fn()
    assert set(a) == set(b)
    for k in sorted(a):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), \
            "%s %s: a second call gives other bits" % (name, k)
    return a


def main(out_path):
    import torch
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = dict(ks=np.array(int(os.environ.get("CLV_LSTM_KS", "4"))))

    def put(tag, inp, got):
        for k, v in inp.items():
            if isinstance(v, np.ndarray):
                out["%s/in/%s" % (tag, k)] = v
        for k, v in got.items():
            out["%s/out/%s" % (tag, k)] = v

    for n, c in enumerate(S.CASES['fwd88']):
        inp = S.forward_inputs(c)
        put("fwd%d" % n, inp, twice("fwd88 %r" % (c,), lambda: forward_once(torch, dev, c, inp)))
    for n, c in enumerate(S.IMPULSE_88):
        for m, scale in enumerate(S.IMPULSE_SCALES):
            inp = S.impulse_inputs(c, scale)
            put("imp%d_%d" % (n, m), inp, twice("impulse %r" % (c,), lambda: forward_once(torch, dev, c, inp)))
    np.savez(out_path, **out)
    print("seq_worker: %d arrays, CLV_LSTM_KS=%s" % (len(out), out['ks']))


if __name__ == "__main__":
    main(sys.argv[1])
