"""-m gpu: the large-batch LSTM kernels (csrc/lstm_mx.hip: clv_lstm_mx_fwd / _bwd) called directly, every output against the
fp64 reference of tests/mx_reference.py -- per element at the pair test's bounds and per slice (batch row, time step, gate or
record slot, the 12-unit block a forward wave owns).  The comparisons, their constants and the inputs are those of
mx_reference.py; tests/test_mx_reference.py shows on the CPU that each of them fails on a planted fault.

Every output buffer is NaN before the launch and followed by canaries; the padding columns of X and Z (ldx > nx, ldz > nz)
hold NaN (byte frames: 255), those of dZ (lddz > nz) canaries.  The backward pass is checked against reference (b) -- BPTT
from the kernel's OWN records, no exemptions -- and end to end against the oracle's BPTT (a); with hard-sigmoid gates (a)
leaves out the elements whose fp64 pre-activation lies within DELTA of a kink, at most KINK_SHARE of a case and
KINK_PER_SLICE of a (row, step): the counts are printed.  The exactness probes print their errors next to the bounds.

Template instances and the case that launches each (hs = hard sigmoid, s = sigmoid; forward <GATE, HASZ, XMODE>, XMODE 0 no
frames, 1 float frames, 2 byte frames; backward <ZT>, ZT = 0 / 1 / 2 for nz = 0 / 1..16 / 17..32):
  fwd <hs,0,1>  test_mx_matches_the_fp64_reference[hs-f32-T1], test_mx_exact_recurrent_product
  fwd <hs,1,2>  ... [hs-z1-u8-T2], test_mx_note_count_ladder[u8-*] (odd rotations)
  fwd <hs,1,0>  ... [hs-z15-T3], [hs-z32-T2], test_mx_exact_latent_product
  fwd <s,1,1>   ... [s-z16-f32-T4]
  fwd <s,1,2>   ... [s-z17-u8-T5]          (rowbias = NULL)
  fwd <s,1,0>   ... [s-z31-T8]
  fwd <hs,1,1>  ... [hs-z32-f32-T9], test_mx_note_count_ladder[f32-*] (odd rotations)
  fwd <s,0,2>   ... [s-u8-T131]
  fwd <hs,0,2>  ... [hs-u8-B1029], test_mx_note_count_ladder[u8-*] (even rotations)
  fwd <hs,0,0>  ... [hs-none-T12]          (nx = nz = 0)
  fwd <s,0,0>   ... [s-none-T2]            (nx = nz = 0)
  fwd <s,0,1>   ... [s-f32-T9]             (rowbias = NULL)
  bwd <0>       nz = 0: [hs-f32-T1], [s-u8-T131], [hs-u8-B1029], [hs-none-T12], [s-none-T2], [s-f32-T9], crafted records
  bwd <1>       nz = 1, 15, 16: [hs-z1-u8-T2], [hs-z15-T3], [s-z16-f32-T4], crafted records
  bwd <2>       nz = 17, 31, 32: [s-z17-u8-T5], [s-z31-T8], [hs-z32-f32-T9], [hs-z32-T2], crafted records, the exactness probes
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mx_reference as MR
from helpers import Bufs

pytestmark = pytest.mark.gpu

H, G4 = MR.H, MR.G4


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def F(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def padded(a, pad, fill, dev, u8=False):
    """rows of a [R,n] with `pad` poisoned columns behind them"""
    a = np.asarray(a)
    out = np.full((a.shape[0], a.shape[1] + pad), fill, np.uint8 if u8 else np.float32)
    out[:, :a.shape[1]] = a
    return torch.as_tensor(out, device=dev)


def run_fwd(c, dev, bufs):
    """one clv_lstm_mx_fwd launch on case c; returns (hs, coef, aux) tensors"""
    from clvae_amd import ops
    B, T, nx, nz = c['B'], c['T'], c['nx'], c['nz']
    u8 = c['kind'] == 'u8'
    Xd = padded(c['X'], 4, 255 if u8 else np.nan, dev, u8) if nx else None
    Zd = padded(c['Z'], 3, np.nan, dev) if nz else None
    hs, coef, aux = bufs.out(B * T, H), bufs.out(B * T, G4), bufs.out(B * T, 2 * H)
    ops.lstm_mx_fwd(B, T, Xd, nx + 4, nx, F(c['Kx'], dev) if nx else None, Zd, nz + 3, nz, F(c['Kz'], dev) if nz else None,
                    F(c['rb'], dev) if c['rb'] is not None else None, F(c['U'], dev), hs, coef, aux,
                    gate_act=0 if c['gate_act'] == MR.HS else 1)
    return hs, coef, aux


def run_bwd(c, dev, bufs, coef, aux, dhs=None):
    """clv_lstm_mx_bwd on a CLONE of the records coef (it becomes dz in place); returns (dz, dzsum, dZ) as numpy, dZ's valid
    columns"""
    from clvae_amd import ops
    B, T, nz = c['B'], c['T'], c['nz']
    dz = bufs.inp(N(coef) if torch.is_tensor(coef) else coef).view(B * T, G4)
    auxd = aux if torch.is_tensor(aux) else F(aux, dev)
    dzsum = bufs.out(B, G4)
    dZ = bufs.out(B * T, nz + 2, pad_cols=2) if nz else None
    ops.lstm_mx_bwd(B, T, F(c['U'], dev), F(c['dhs'] if dhs is None else dhs, dev), auxd, dz, dzsum,
                    Kz=F(c['Kz'], dev) if nz else None, nz=nz, dZ=dZ, lddz=nz + 2)
    torch.cuda.synchronize()
    return N(dz), N(dzsum), N(dZ)[:, :nz] if nz else None


def check_pass(c, dev, bufs, name):
    """forward against fp64, backward against (b) on the launch's own records and against (a)"""
    B, T = c['B'], c['T']
    hs, coef, aux = run_fwd(c, dev, bufs)
    torch.cuda.synchronize()
    nex = MR.check_forward(c['ref'], N(hs), N(coef).reshape(B * T, H, 4), N(aux).reshape(B * T, H, 2), name + ' ')
    dz, dzsum, dZ = run_bwd(c, dev, bufs, coef, aux)
    b = MR.backward_coef(N(coef).reshape(B * T, H, 4), N(aux).reshape(B * T, H, 2), c['dhs'], c['U'], c['Kz'])
    MR.check_backward(b, dz, dzsum, dZ, Kz=c['Kz'], name=name + ' (b) ')
    a = MR.backward_oracle(c['ref'], c['dhs'], c['U'], c['Kz'])
    if c['gate_act'] == MR.HS:
        MR.check_backward(a, dz, dzsum, dZ, Kz=c['Kz'], name=name + ' (a) ', slices=False,
                          exclude=MR.kink_exclusions(c['ref']['pre'], MR.HS))
    else:
        MR.check_backward(a, dz, dzsum, dZ, Kz=c['Kz'], name=name + ' (a) ', slices=False)
    return nex


@pytest.mark.parametrize("cid", list(MR.CASES))
def test_mx_matches_the_fp64_reference(dev, cid):
    """a, c, d, g: every forward instance and every backward instance, T = 1 .. 5 and 131, B = 1 .. 5, 9 and 1029, nz on both
    sides of the backward dispatch, nx = 1, 5, 7, 95, byte frames against fp64, rowbias = NULL twice"""
    c = MR.case(cid)
    bufs = Bufs(dev)
    nex = check_pass(c, dev, bufs, "%s seed %d" % (cid, c['seed']))
    bufs.check_canaries()
    print("%s: %d of %d coefficients within %.0e of a kink left out (cap %d, %d per (row, step))" % (
        cid, nex, c['ref']['gates'].size, MR.DELTA, int(MR.KINK_SHARE * c['ref']['gates'].size), MR.KINK_PER_SLICE))


@pytest.mark.parametrize("nx", MR.LADDER_NX)
@pytest.mark.parametrize("kind", ['f32', 'u8'])
def test_mx_note_count_ladder(dev, kind, nx):
    """b: frames of exactly 0, 1, 4, 5, 8, 9, 12, 15, 16, 17, 19, 20, nx - 1 and nx notes (the two unrolled rounds, the
    one-at-a-time tail, the padded tail, the empty and the full frame), each count at every step of every row of a full
    workgroup and of the single row of a partial one (one launch per rotation); float frames with negative and
    fractional values and -0.0 for off, byte frames with values up to 255.  Along a row the counts follow
    MR.ladder_order: where a list's padding belongs, the list two steps earlier left a real note"""
    total = 0
    for rot in range(len(MR.ladder_counts(nx))):
        c = MR.ladder_case(nx, kind, rot)
        bufs = Bufs(dev)
        total += check_pass(c, dev, bufs, "nx %d rotation %d seed %d" % (nx, rot, c['seed']))
        bufs.check_canaries()
    print("ladder nx %d %s: counts %s, %d coefficients near a kink left out in all" % (nx, kind, MR.ladder_counts(nx), total))


@pytest.mark.parametrize("B,T,nz,seed", [(5, 6, 0, 1), (9, 9, 16, 2), (3, 3, 17, 3), (4, 8, 32, 4), (2, 1, 1, 5)])
def test_mx_bwd_on_crafted_records(dev, B, T, nz, seed):
    """e: records no forward pass would write (the pass is linear in them): signs everywhere, kcarry outside [0, 1], the
    records of some (row, step) all zero"""
    rng = np.random.default_rng(seed)
    c = dict(B=B, T=T, nz=nz, U=MR.f32(MR.O.orthogonal(rng, (H, G4), np.float64) * 1.5),
             Kz=MR.f32(rng.standard_normal((nz, G4)) * 0.4) if nz else None, dhs=MR.f32(rng.standard_normal((B, T, H))))
    coef = MR.f32(rng.standard_normal((B * T, H, 4)) * 0.5)
    aux = MR.f32(np.stack([rng.uniform(-1.2, 1.3, (B * T, H)), rng.standard_normal((B * T, H))], -1))
    dead = rng.random(B * T) < 0.25
    coef[dead], aux[dead] = 0.0, 0.0
    assert (aux[..., 0] > 1).any() and (aux[..., 0] < 0).any()
    bufs = Bufs(dev)
    dz, dzsum, dZ = run_bwd(c, dev, bufs, coef.reshape(B * T, G4), aux.reshape(B * T, 2 * H))
    MR.check_backward(MR.backward_coef(coef, aux, c['dhs'], c['U'], c['Kz']), dz, dzsum, dZ, Kz=c['Kz'])
    assert not dz.reshape(B * T, G4)[dead].any()
    bufs.check_canaries()


def _linear_forget(kcarry, rb_f):
    """z_f - rb_f read back from kcarry = 0.2 z_f + 0.5 (the hard sigmoid's linear part)"""
    assert (kcarry > 0.05).all() and (kcarry < 0.95).all()
    return (kcarry - 0.5) / 0.2 - rb_f


def test_mx_exact_recurrent_product(dev):
    """f, forward h . U: T = 2, the kernel's own h_0 (it depends on the step-0 frames alone), U's forget block coherent with
    the pieces of row 0's h_0 and about 16 x an orthogonal U's entries, rowbias = -fp32(h_0 . U_f) + r on the forget block:
    the hard sigmoid is linear there and kcarry_1 gives the product back to EXACT_BOUND['hU'] + EXACT_READBACK"""
    X, Kx = MR.exact_fwd_step0()
    B = MR.EXACT_B
    rng = np.random.default_rng(21)
    c = dict(B=B, T=2, nx=X.shape[1], nz=0, kind='f32', gate_act=MR.HS, X=X, Kx=Kx, Z=None, Kz=None,
             rb=np.zeros((B, G4)), U=np.zeros((H, G4)))
    bufs = Bufs(dev)
    h0 = N(run_fwd(c, dev, bufs)[0]).reshape(B, 2, H)[:, 0]
    W = MR.exact_probe('hU', h0[0])[1]
    c['U'] = MR.f32(MR.O.orthogonal(rng, (H, G4), np.float64) * 24.0)
    c['U'][:, H:2 * H] = W
    c['rb'][:, H:2 * H] = MR.cancelling(rng, h0 @ W, 2.0)
    hs, _, aux = run_fwd(c, dev, bufs)
    torch.cuda.synchronize()
    assert np.array_equal(N(hs).reshape(B, 2, H)[:, 0], h0)
    got = _linear_forget(N(aux).reshape(B, 2, H, 2)[:, 1, :, 0], c['rb'][:, H:2 * H])
    err = MR.assert_exact('hU', got, h0, W, readback=True)
    bufs.check_canaries()
    print("h . U: largest error %.2e of products up to %.1f, bound %.2e + %.1e" % (
        err, np.abs(h0 @ W).max(), MR.EXACT_BOUND['hU'], MR.EXACT_READBACK))


def test_mx_exact_latent_product(dev):
    """f, forward z . Kz: nx = 0, U's forget block zero, the same read-back through kcarry at step 1"""
    a, W = MR.exact_probe('zKz')
    B, nz = MR.EXACT_B, MR.MX_NZMAX
    rng = np.random.default_rng(22)
    Z = MR.f32(rng.standard_normal((B, 2, nz)))
    Z[:, 1] = a
    c = dict(B=B, T=2, nx=0, nz=nz, kind='f32', gate_act=MR.HS, X=None, Kx=None, Z=Z.reshape(B * 2, nz),
             Kz=MR.f32(rng.standard_normal((nz, G4)) * 0.4), rb=MR.f32(rng.standard_normal((B, G4)) * 0.3),
             U=MR.f32(MR.O.orthogonal(rng, (H, G4), np.float64) * 1.5))
    c['Kz'][:, H:2 * H] = W
    c['U'][:, H:2 * H] = 0.0
    c['rb'][:, H:2 * H] = MR.cancelling(rng, a @ W, 2.0)
    bufs = Bufs(dev)
    _, _, aux = run_fwd(c, dev, bufs)
    torch.cuda.synchronize()
    got = _linear_forget(N(aux).reshape(B, 2, H, 2)[:, 1, :, 0], c['rb'][:, H:2 * H])
    err = MR.assert_exact('zKz', got, a, W, readback=True)
    bufs.check_canaries()
    print("z . Kz: largest error %.2e of products up to %.1f, bound %.2e + %.1e" % (
        err, np.abs(a @ W).max(), MR.EXACT_BOUND['zKz'], MR.EXACT_READBACK))


@pytest.mark.parametrize("kind", ['dzUT', 'dzKzT'])
def test_mx_exact_backward_products(dev, kind):
    """f, backward: records ki = kc = 1 and nothing else, T = 2: dz_i[1] = dhs[1] and dz_i[0] = dhs[0] + dz[1] . U^T, with
    dhs[0] = -fp32(dz[1] . U^T) + a small rest the product's error is what is left; dZ[1] = dz[1] . Kz^T is read directly"""
    a, W = MR.exact_probe(kind)
    B, nz = MR.EXACT_B, MR.MX_NZMAX
    rng = np.random.default_rng(23)
    c = dict(B=B, T=2, nz=nz, U=MR.f32(MR.O.orthogonal(rng, (H, G4), np.float64) * 1.5),
             Kz=MR.f32(rng.standard_normal((nz, G4)) * 0.4))
    if kind == 'dzUT':
        c['U'][:, :H] = W.T
    else:
        c['Kz'][:, :H] = W.T
    rec = a @ c['U'][:, :H].T
    dhs = np.stack([MR.cancelling(rng, rec, 1e-2), a], 1)
    coef, aux = np.zeros((B * 2, H, 4)), np.zeros((B * 2, H, 2))
    coef[..., 0], aux[..., 1] = 1.0, 1.0
    bufs = Bufs(dev)
    dz, dzsum, dZ = run_bwd(c, dev, bufs, coef.reshape(B * 2, G4), aux.reshape(B * 2, 2 * H), dhs=dhs)
    dz = dz.reshape(B, 2, G4)
    assert np.array_equal(dz[:, 1, :H], a) and not dz[:, :, H:].any()
    if kind == 'dzUT':
        err = MR.assert_exact(kind, dz[:, 0, :H] - dhs[:, 0], a, W)
    else:
        err = MR.assert_exact(kind, dZ.reshape(B, 2, nz)[:, 1], a, W)
    np.testing.assert_allclose(dzsum.reshape(B, G4)[:, :H], dz[:, 0, :H] + dz[:, 1, :H], rtol=2.0 ** -23, atol=0)     # one fp32 sum
    bufs.check_canaries()
    print("%s: largest error %.2e of products up to %.1f, bound %.2e" % (kind, err, np.abs(a @ W).max(), MR.EXACT_BOUND[kind]))


def test_mx_refusals(dev):
    """h: CLV_EINVAL for records that are not 16- / 8-byte aligned, nx = 97, nz = 33, ldx < nx, ldz < nz, lddz < nz; nothing
    is launched: every output stays NaN"""
    from clvae_amd import _lib, ops
    B, T, nx, nz = 3, 2, 88, 4
    z = lambda *sh: torch.zeros(*sh, device=dev)
    bufs = Bufs(dev)
    hs, coef, aux, dzsum, dZ = bufs.out(B * T, H), bufs.out(B * T * G4 + 4), bufs.out(B * T * 2 * H + 4), bufs.out(B, G4), bufs.out(B * T, 40)
    co, au = coef[:B * T * G4].view(B * T, G4), aux[:B * T * 2 * H].view(B * T, 2 * H)
    co1, au1 = coef[1:B * T * G4 + 1].view(B * T, G4), aux[1:B * T * 2 * H + 1].view(B * T, 2 * H)
    assert co1.data_ptr() % 16 == 4 and au1.data_ptr() % 8 == 4 and co.data_ptr() % 16 == 0
    X, Kx, Z, Kz, rb, U, dhs = z(B * T, 100), z(100, G4), z(B * T, 40), z(40, G4), z(B, G4), z(H, G4), z(B * T, H)

    def fwd(co=co, au=au, nx=nx, ldx=100, nz=nz, ldz=40):
        ops.lstm_mx_fwd(B, T, X, ldx, nx, Kx, Z, ldz, nz, Kz, rb, U, hs, co, au)

    def bwd(co=co, au=au, nz=nz, lddz=40):
        ops.lstm_mx_bwd(B, T, U, dhs, au, co, dzsum, Kz=Kz, nz=nz, dZ=dZ, lddz=lddz)

    for call, kw in [(fwd, dict(co=co1)), (fwd, dict(au=au1)), (fwd, dict(nx=97)), (fwd, dict(nz=33)), (fwd, dict(ldx=87)),
                     (fwd, dict(ldz=3)), (bwd, dict(co=co1)), (bwd, dict(au=au1)), (bwd, dict(nz=33)), (bwd, dict(lddz=3))]:
        with pytest.raises(_lib.ClvError, match=r"\(-1\)"):
            call(**kw)
    torch.cuda.synchronize()
    for t in (hs, coef, aux, dzsum, dZ):
        assert torch.isnan(t).all()
    bufs.check_canaries()
