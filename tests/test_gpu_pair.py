"""-m gpu: the pair kernels (csrc/lstm_pair.hip: clv_lstm_pair_pack / _fwd / _bwd) called directly, every output against the
fp64 reference of tests/pair_reference.py, per element and per slice (batch row, time step, gate block, latent column).

Every output buffer is filled with NaN before each launch and followed by canary values; Z has canary padding columns
(ldz > L).  The backward pass is checked tightly against reference (b) -- BPTT driven by the kernel's OWN forward records --
and, where the gates are smooth (sigmoid), also end to end against the oracle's BPTT (a): with hard-sigmoid gates an fp32
pre-activation on the other side of a kink than its fp64 value changes one coefficient by 0.2 and every earlier dz with it.
All 28 instances below ran in one `rocprofv3 --kernel-trace --stats` pass over this file.

Template instances and the case that launches each (hs = hard sigmoid, s = sigmoid; forward <G, dec_has_xproj, Z, XL>,
Z = 1 for L <= 4 and 2 for L 5..8; backward <G, ZP, WZG>, ZP = 4 / 8 / 16 for L <= 2 / 3..4 / 5..8):
  fwd <hs,1,1,0>  test_pair_matches_the_fp64_reference[3-7-1-hard_sigmoid-True-*], [1024-2-2-...]
  fwd <s,0,1,0>   ... [257-4-2-sigmoid-False-*]
  fwd <hs,0,1,0>  ... [1-1-3-hard_sigmoid-False-*]
  fwd <s,1,1,0>   ... [256-2-4-sigmoid-True-*]
  fwd <hs,1,2,0>  ... [3-3-5-hard_sigmoid-True-*]
  fwd <s,0,2,0>   ... [4-128-8-sigmoid-False-*]
  fwd <hs,0,2,0>  ... [5-4-6-hard_sigmoid-False-*]
  fwd <s,1,2,0>   ... [2-7-7-sigmoid-True-*]
  fwd <G,X,Z,1>   test_pair_note_lists_match_the_dense_projections[G-X-L], L = 2 (Z = 1) and 6 (Z = 2): all 8
  bwd <hs,4,1>  L = 1, <s,4,1> L = 2, <hs,8,1> L = 3, <s,8,1> L = 4, <hs,16,1> L = 5, 6, <s,16,1> L = 7, 8:
                  test_pair_matches_the_fp64_reference
  bwd <G,ZP,0>    test_pair_bwd_without_head_grad_is_the_same_pass[L-G]: all 6
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import clvae_oracle as O
from oracle import philox as OP
import pair_reference as PR
from helpers import Bufs

pytestmark = pytest.mark.gpu

H, G4 = PR.H, PR.G4
KL_SCALE = 0.37
DELTA = 1e-4            # hard-sigmoid coefficients against the fp64 forward: elements this close to a kink are left out
SLICE_RTOL, SLICE_ATOL = PR.SLICE_RTOL, PR.SLICE_ATOL       # per-slice bounds: see pair_reference.py


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def sliced(got, ref, axes, name, exclude=None, rtol=SLICE_RTOL):
    ref = np.asarray(ref, np.float64)
    return PR.assert_close_sliced(got, ref, axes, SLICE_ATOL * max(np.abs(ref).max(), 1e-30), rtol, exclude=exclude,
                                  name=name)


def make_case(B, Tn, L, gate, xp_dec, seed, dhs_mode='dense'):
    """inputs (fp32 values) and the fp64 reference forward.  The input projections are dense N(0, 2.2^2): with the per-row
    bias and the recurrent term about 28 % of the gate pre-activations lie beyond the hard sigmoid's kinks."""
    rng = np.random.default_rng(seed)
    c = dict(B=B, T=Tn, L=L, gate=gate, xp_dec=xp_dec)
    c['Ue'] = f32(O.orthogonal(rng, (H, G4), np.float64))
    c['Ud'] = f32(O.orthogonal(rng, (H, G4), np.float64))
    c['Kz'] = f32(rng.standard_normal((L, G4)) * 0.5)
    c['Wz'] = f32(rng.standard_normal((H, 2 * L)) * 0.3)
    c['bz'] = f32(rng.standard_normal(2 * L) * 0.2)
    c['xe'] = f32(rng.standard_normal((B, Tn, G4)) * 2.2)
    c['xd'] = f32(rng.standard_normal((B, Tn, G4)) * 2.2) if xp_dec else None
    c['rbe'] = f32(rng.standard_normal((B, G4)) * 0.5)
    c['rbd'] = f32(rng.standard_normal((B, G4)) * (0.5 if xp_dec else 2.2))
    c['eps'] = f32(rng.standard_normal((B, Tn, L)))
    dhs = f32(rng.standard_normal((B, Tn, H)))
    if dhs_mode == 'last':          # every earlier dz of both chains is a pure carry through the skew and the latent head
        dhs[:, :-1] = 0.0
    c['dhs'] = dhs
    c['ref'] = PR.pair_forward(c['xe'], c['xd'], c['rbe'], c['rbd'], c['Ue'], c['Ud'], c['Kz'], c['Wz'], c['bz'], c['eps'],
                               gate)
    return c


def run_pack(c, dev, bufs):
    from clvae_amd import ops
    pack = bufs.out(ops.lstm_pair_pack_floats())
    ops.lstm_pair_pack(c['L'], T(c['Ue'], dev), T(c['Ud'], dev), T(c['Kz'], dev), T(c['Wz'], dev), pack)
    return pack


def run_fwd(c, dev, bufs, pack, gates=None, notes=None, noise=None, eps=None):
    """one clv_lstm_pair_fwd launch; returns its outputs (gates_* = the coefficient records)"""
    from clvae_amd import ops
    B, Tn, L = c['B'], c['T'], c['L']
    BT, ldz = B * Tn, L + 3
    if gates is None:
        gates = (bufs.inp(c['xe']).view(BT, G4), bufs.inp(c['xd']).view(BT, G4) if c['xp_dec'] else bufs.out(BT, G4))
    o = dict(gates_enc=gates[0], gates_dec=gates[1])
    o['eps'] = eps if eps is not None else bufs.inp(c['eps'])
    for k, shape in (('hs_enc', (BT, H)), ('aux_enc', (BT, 2 * H)), ('hs_dec', (BT, H)), ('aux_dec', (BT, 2 * H)),
                     ('zargs', (BT, 2 * L)), ('klterm', (BT, L))):
        o[k] = bufs.out(*shape)
    o['Z'] = bufs.out(BT, ldz, pad_cols=ldz - L)
    ops.lstm_pair_fwd(B, Tn, L, o['gates_enc'], T(c['rbe'], dev), o['gates_dec'], c['xp_dec'], T(c['rbd'], dev), pack,
                      T(c['bz'], dev), o['eps'], o['hs_enc'], o['aux_enc'], o['hs_dec'], o['aux_dec'], o['zargs'], o['Z'], ldz,
                      o['klterm'], gate_act=0 if c['gate'] == 'hard_sigmoid' else 1, noise=noise, notes=notes)
    return o


def run_bwd(c, dev, bufs, pack, f, head_grad=True, defer=None, label=None, kl=KL_SCALE):
    """clv_lstm_pair_bwd on CLONES of the forward records (the gate buffers become dz in place)"""
    from clvae_amd import ops
    B, Tn, L = c['B'], c['T'], c['L']
    BT = B * Tn
    r = dict(dz_dec=bufs.inp(N(f['gates_dec'])), dz_enc=bufs.inp(N(f['gates_enc'])))
    r['dzsum_dec'], r['dzsum_enc'], r['dzargs'] = bufs.out(B, G4), bufs.out(B, G4), bufs.out(BT, 2 * L)
    r['dWz'], r['dbz'] = bufs.out(H, 2 * L), bufs.out(2 * L)
    hg = (f['hs_enc'], r['dWz'], r['dbz']) if head_grad else None
    ops.lstm_pair_bwd(B, Tn, L, kl, pack, T(c['Wz'], dev), T(c['dhs'], dev), f['aux_dec'], f['aux_enc'], r['dz_dec'],
                      r['dz_enc'], r['dzsum_dec'], r['dzsum_enc'], f['zargs'], f['eps'], r['dzargs'],
                      gate_act=0 if c['gate'] == 'hard_sigmoid' else 1, head_grad=hg, ws=ops.Workspace(dev), defer=defer,
                      label=label)
    return r


def check_forward(c, f, ref=None):
    """every forward output of launch f against the fp64 reference: per element at the bounds of the lstm_mx and latent
    head tests, and per slice"""
    B, Tn, L, gate = c['B'], c['T'], c['L'], c['gate']
    ref = ref or c['ref']
    assert np.isfinite(N(f['gates_enc'])).all() and np.isfinite(N(f['gates_dec'])).all()
    for ch in ('enc', 'dec'):
        hs = N(f['hs_' + ch]).reshape(B, Tn, H)
        np.testing.assert_allclose(hs, ref['hs_' + ch], atol=5e-6, err_msg='hs_' + ch)
        sliced(hs, ref['hs_' + ch], (0, 1), 'hs_' + ch)
        # coefficients: hard-sigmoid derivatives whose fp64 pre-activation is within DELTA of a kink are left out
        got = N(f['gates_' + ch]).reshape(B, Tn, G4)
        want = ref['gates_' + ch]
        ex = PR.kink_mask(ref['pre_' + ch], gate, DELTA)
        assert (np.abs(got - want)[~ex] <= 2e-5 * (1 + np.abs(want[~ex]))).all(), 'gates_' + ch
        nex = sliced(got.reshape(B, Tn, 4, H), want.reshape(B, Tn, 4, H), (0, 1, 2), 'gates_' + ch,
                     exclude=ex.reshape(B, Tn, 4, H))
        print("gates_%s: %d of %d coefficients within %.0e of a kink left out" % (ch, nex, got.size, DELTA))
        ga, wa = N(f['aux_' + ch]).reshape(B, Tn, 2, H), ref['aux_' + ch].reshape(B, Tn, 2, H)
        np.testing.assert_allclose(ga[:, :, 0], wa[:, :, 0], atol=5e-6, err_msg='kcarry_' + ch)
        np.testing.assert_allclose(ga[:, :, 1], wa[:, :, 1], atol=1e-5, err_msg='kc_' + ch)
        sliced(ga, wa, (0, 1, 2), 'aux_' + ch)
    # the latent head, from the kernel's own encoder states (the latent head test's bounds)
    za, Z, kt = PR.latent_forward(N(f['hs_enc']).reshape(B, Tn, H), c['Wz'], c['bz'], N(f['eps']).reshape(B, Tn, L))
    np.testing.assert_allclose(N(f['zargs']).reshape(B, Tn, 2 * L), za, rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(N(f['Z'])[:, :L].reshape(B, Tn, L), Z, rtol=1e-5, atol=3e-5)
    np.testing.assert_allclose(N(f['klterm']).reshape(B, Tn, L), kt, rtol=2e-5, atol=2e-4)
    sliced(N(f['zargs']).reshape(B, Tn, 2 * L), za, (0, 1, 2), 'zargs')
    sliced(N(f['Z'])[:, :L].reshape(B, Tn, L), Z, (0, 1, 2), 'Z')
    sliced(N(f['klterm']).reshape(B, Tn, L), kt, (0, 1, 2), 'klterm')
    # ... and end to end
    np.testing.assert_allclose(N(f['zargs']).reshape(B, Tn, 2 * L), ref['zargs'], rtol=1e-5, atol=5e-5)


def check_backward(c, f, r, head_grad=True):
    """the backward launch r against reference (b) on the forward records of launch f"""
    B, Tn, L = c['B'], c['T'], c['L']
    rec = lambda k, *sh: N(f[k]).reshape(*sh)
    ref = PR.pair_backward_coef(rec('gates_enc', B, Tn, G4), rec('aux_enc', B * Tn, 2, H), rec('gates_dec', B, Tn, G4),
                                rec('aux_dec', B * Tn, 2, H), rec('zargs', B, Tn, 2 * L), rec('hs_enc', B, Tn, H), c['dhs'],
                                c['Ue'], c['Ud'], c['Kz'], c['Wz'], rec('eps', B, Tn, L), KL_SCALE)
    for ch in ('dec', 'enc'):
        dz, want = N(r['dz_' + ch]).reshape(B, Tn, G4), ref['dz_' + ch]
        assert (np.abs(dz - want) <= 3e-5 * (1 + np.abs(want))).all(), 'dz_' + ch
        sliced(dz.reshape(B, Tn, 4, H), want.reshape(B, Tn, 4, H), (0, 1, 2), 'dz_' + ch)
        ds = N(r['dzsum_' + ch])
        np.testing.assert_allclose(ds, dz.sum(1), atol=2e-4, err_msg='dzsum_' + ch)
        sliced(ds.reshape(B, 4, H), ref['dzsum_' + ch].reshape(B, 4, H), (0, 1), 'dzsum_' + ch)
    dza = N(r['dzargs']).reshape(B, Tn, 2 * L)
    np.testing.assert_allclose(dza, ref['dzargs'], rtol=2e-5, atol=2e-5)
    sliced(dza, ref['dzargs'], (0, 1, 2), 'dzargs')
    if head_grad:
        np.testing.assert_allclose(N(r['dWz']), ref['dWz'], rtol=1e-4, atol=2e-5 * max(1.0, np.abs(ref['dWz']).max()))
        np.testing.assert_allclose(N(r['dbz']), ref['dbz'], rtol=1e-4, atol=2e-5 * max(1.0, np.abs(ref['dbz']).max()))
        sliced(N(r['dWz']), ref['dWz'], (0, 1), 'dWz')
        sliced(N(r['dbz']), ref['dbz'], (0,), 'dbz')
    return ref


MAIN = [  # B, T, L, gate, dec_has_xproj
    (3, 7, 1, 'hard_sigmoid', True),
    (257, 4, 2, 'sigmoid', False),
    (1, 1, 3, 'hard_sigmoid', False),
    (256, 2, 4, 'sigmoid', True),
    (3, 3, 5, 'hard_sigmoid', True),
    (4, 128, 8, 'sigmoid', False),
    (5, 4, 6, 'hard_sigmoid', False),
    (2, 7, 7, 'sigmoid', True),
    (1024, 2, 2, 'hard_sigmoid', True),        # more rows than CUs: four rounds of workgroups
]


@pytest.mark.parametrize("dhs_mode", ['dense', 'last'])
@pytest.mark.parametrize("B,Tn,L,gate,xp_dec", MAIN)
def test_pair_matches_the_fp64_reference(dev, B, Tn, L, gate, xp_dec, dhs_mode):
    """pack, forward and backward (with the latent head's weight gradient) at once; odd / even T from 1 to 128, batches of
    1 to 1024 rows, latent_dim 1 to 8; upstream dL/dh_dec dense or only at the last step."""
    c = make_case(B, Tn, L, gate, xp_dec, B * 1000 + Tn * 10 + L, dhs_mode)
    if gate == 'hard_sigmoid':       # the zero-derivative branch is exercised
        for ch in ('enc', 'dec'):
            sat = PR.saturated_fraction(c['ref']['pre_' + ch])
            assert 0.2 <= sat <= 0.4, (ch, sat)
    bufs = Bufs(dev)
    pack = run_pack(c, dev, bufs)
    f = run_fwd(c, dev, bufs, pack)
    torch.cuda.synchronize()
    check_forward(c, f)
    r = run_bwd(c, dev, bufs, pack, f)
    torch.cuda.synchronize()
    check_backward(c, f, r)
    bufs.check_canaries()
    if gate == 'sigmoid' and dhs_mode == 'dense':
        # once end to end against the oracle's BPTT (smooth gates: no coefficient sits on a kink), the lstm_mx bound
        a = PR.pair_backward_oracle(c['ref'], c['dhs'], c['Ue'], c['Ud'], c['Kz'], c['Wz'], c['eps'], KL_SCALE)
        for ch in ('dec', 'enc'):
            dz = N(r['dz_' + ch]).reshape(B, Tn, G4)
            assert (np.abs(dz - a['dz_' + ch]) <= 3e-5 * (1 + np.abs(a['dz_' + ch]))).all(), 'dz_' + ch
        np.testing.assert_allclose(N(r['dzargs']).reshape(B, Tn, 2 * L), a['dzargs'], rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("L,gate", [(2, 'hard_sigmoid'), (4, 'hard_sigmoid'), (8, 'hard_sigmoid'), (1, 'sigmoid'),
                                    (3, 'sigmoid'), (6, 'sigmoid')])
def test_pair_bwd_without_head_grad_is_the_same_pass(dev, L, gate):
    """head_grad=None (WZG = false): dWz / dbz are not written, and every other output is bit for bit the WZG = true run"""
    c = make_case(3, 5, L, gate, True, 77 + L)
    bufs = Bufs(dev)
    pack = run_pack(c, dev, bufs)
    f = run_fwd(c, dev, bufs, pack)
    r1 = run_bwd(c, dev, bufs, pack, f, head_grad=True)
    r0 = run_bwd(c, dev, bufs, pack, f, head_grad=False)
    torch.cuda.synchronize()
    check_backward(c, f, r0, head_grad=False)
    for k in ('dz_dec', 'dz_enc', 'dzsum_dec', 'dzsum_enc', 'dzargs'):
        assert torch.equal(r0[k], r1[k]), k
    assert torch.isnan(r0['dWz']).all() and torch.isnan(r0['dbz']).all()
    bufs.check_canaries()


def _frames(rng, B, Tn, density):
    X = (rng.random((B * Tn, 88)) < density).astype(np.uint8)
    X[0] = 0                    # an empty frame
    X[1 % (B * Tn)] = 1         # all 88 notes
    X[2 % (B * Tn)] = 0
    X[2 % (B * Tn), rng.permutation(88)[:13]] = 1        # more than 8 notes: the kernel's one-at-a-time tail
    return X


@pytest.mark.parametrize("L", [2, 6])
@pytest.mark.parametrize("xp_dec", [True, False])
@pytest.mark.parametrize("gate", ['hard_sigmoid', 'sigmoid'])
def test_pair_note_lists_match_the_dense_projections(dev, gate, xp_dec, L):
    """notes=...: the input projections gathered inside the forward kernel from ops.gather_rows_multi note lists (an empty
    frame, a full one, one of 13 notes, one list reversed) against the same launch fed the dense projections of
    ops.sparse_proj2.  Not bit for bit: the kernel sums a frame's first 8 kernel rows as a tree and the rest in list order,
    sparse_proj in ascending note order -- so within fp32 rounding of the projections, and both against the fp64 reference."""
    from clvae_amd import ops
    B, Tn = 3, 5
    rng = np.random.default_rng(L * 10 + xp_dec)
    Xe, Xd = _frames(rng, B, Tn, 0.1), _frames(rng, B, Tn, 0.1)[::-1].copy()
    Ke, Kd = f32(rng.standard_normal((88, G4)) * 0.9), f32(rng.standard_normal((88, G4)) * 0.9)
    c = make_case(B, Tn, L, gate, xp_dec, 300 + L)
    c['xe'] = (Xe.astype(np.float64) @ Ke).reshape(B, Tn, G4)
    c['xd'] = (Xd.astype(np.float64) @ Kd).reshape(B, Tn, G4) if xp_dec else None
    c['ref'] = PR.pair_forward(c['xe'], c['xd'], c['rbe'], c['rbd'], c['Ue'], c['Ud'], c['Kz'], c['Wz'], c['bz'], c['eps'],
                               gate)
    BT = B * Tn
    de, dd = torch.as_tensor(Xe, device=dev), torch.as_tensor(Xd, device=dev)
    fe, fd = torch.empty(BT, 88, device=dev), torch.empty(BT, 88, device=dev)
    ne = torch.full((BT, ops.NOTE_ROW), ops.NOTE_NONE, dtype=torch.uint8, device=dev)
    nd = ne.clone()
    ops.gather_rows_multi(BT, None, [(de, fe, 88, 88, 88), (dd, fd, 88, 88, 88)], notes=[ne, nd])
    torch.cuda.synchronize()
    full = int(np.flatnonzero(Xe.sum(1) == 13)[0])         # reverse the 13-note list of the encoder's frames
    row = ne[full].cpu().numpy()
    assert sorted(row[:13].tolist()) == np.flatnonzero(Xe[full]).tolist()
    row[:13] = row[:13][::-1].copy()
    ne[full] = torch.as_tensor(row, device=dev)
    bufs = Bufs(dev)
    pack = run_pack(c, dev, bufs)
    Ked, Kdd = T(Ke, dev), T(Kd, dev)
    g_e, g_d = bufs.out(BT, G4), bufs.out(BT, G4)
    if xp_dec:
        ops.sparse_proj2(BT, G4, (88, de, 88, Ked, g_e), (88, dd, 88, Kdd, g_d))
    else:
        ops.sparse_proj(BT, 88, G4, de, 88, Ked, g_e)
    dense = run_fwd(c, dev, bufs, pack, gates=(g_e, g_d))
    lists = run_fwd(c, dev, bufs, pack, gates=(bufs.out(BT, G4), bufs.out(BT, G4)),
                    notes=(ne, Ked, nd if xp_dec else None, Kdd if xp_dec else None))
    torch.cuda.synchronize()
    check_forward(c, dense)
    check_forward(c, lists)
    for k in ('hs_enc', 'hs_dec', 'zargs', 'Z', 'klterm'):
        np.testing.assert_allclose(N(lists[k]), N(dense[k]), rtol=1e-5, atol=5e-6, err_msg=k)
    bufs.check_canaries()


def test_pair_draws_its_own_noise(dev):
    """noise=...: eps drawn in the forward kernel's prologue is the Philox normal at (seed, step + *step_dev, stream,
    first + b*T*L + t*L + l) -- oracle/philox.py to libm precision, ops.philox_normal bit for bit -- and the pass is bit for
    bit the one fed that eps from the host"""
    from clvae_amd import ops
    B, Tn, L = 5, 7, 3
    seed, stream, step, first = 0x1234567890AB, 7, 3, 1000
    c = make_case(B, Tn, L, 'hard_sigmoid', True, 9)
    bufs = Bufs(dev)
    pack = run_pack(c, dev, bufs)
    it = torch.tensor([2], dtype=torch.int32, device=dev)
    nz = ops.noise_draw(seed, stream, first, step - 2, it)
    drawn = run_fwd(c, dev, bufs, pack, noise=nz, eps=bufs.out(B, Tn, L))
    ref = torch.empty(B * Tn * L, dtype=torch.float32, device=dev)
    ops.philox_normal(ref, B * Tn * L, seed, step, stream, first)
    torch.cuda.synchronize()
    want = OP.normal(B * Tn * L, seed, step=step, stream_id=stream, first_index=first).reshape(B, Tn, L)
    np.testing.assert_allclose(N(drawn['eps']), want, atol=2e-5)
    assert torch.equal(drawn['eps'].reshape(-1), ref)
    host = run_fwd(c, dev, bufs, pack, eps=bufs.inp(N(drawn['eps'])))
    torch.cuda.synchronize()
    for k in ('gates_enc', 'gates_dec', 'hs_enc', 'aux_enc', 'hs_dec', 'aux_dec', 'zargs', 'Z', 'klterm'):
        assert torch.equal(drawn[k], host[k]), k
    c['eps'] = N(drawn['eps'])
    c['ref'] = PR.pair_forward(c['xe'], c['xd'], c['rbe'], c['rbd'], c['Ue'], c['Ud'], c['Kz'], c['Wz'], c['bz'], c['eps'],
                               c['gate'])
    check_forward(c, drawn)
    bufs.check_canaries()


def _label_inputs(rng, B, Cn, D=88):
    C1 = Cn - 1
    wargs = f32(rng.standard_normal((B, 2 * C1)) * 0.5)
    eps_w = f32(rng.standard_normal((B, C1)))
    W = f32(O.logistic_normal(wargs[:, :C1], wargs[:, C1:], eps_w))
    hW = f32(np.maximum(rng.standard_normal((B, D)), 0))
    return dict(D=D, C=Cn, Kenc_w=f32(rng.standard_normal((Cn, G4)) * 0.1), Kdec_w=f32(rng.standard_normal((Cn, G4)) * 0.1),
                wargs=wargs, eps=eps_w, onehot=np.eye(Cn)[rng.integers(0, Cn, B)], W=W, hW=hW,
                Ka=f32(rng.standard_normal((D, 2 * C1)) * 0.2), prior=0.2, class_weight=0.8, w_kl_weight=0.9, inv_b=1.0 / B)


@pytest.mark.parametrize("B,layer_grad,defer", [(1, True, True), (1, False, False), (6, True, False), (6, True, True),
                                                (6, False, True)])
def test_pair_label_rider_is_vrnn_label_bwd(dev, B, layer_grad, defer):
    """label=...: the label path's backward as the pair backward kernel's epilogue is clv_vrnn_label_bwd on the same dzsum
    (the header: "same arithmetic, same outputs") -- bit for bit -- and the fp64 label backward; the latent head's weight
    gradient deferred to a ReduceQueue is bit for bit the immediate one (B = 1: the kernel ignores the job and reduces at
    once)."""
    from clvae_amd import ops
    Cn, D = 5, 88
    c = make_case(B, 6, 3, 'hard_sigmoid', True, 50 + B)
    lab = _label_inputs(np.random.default_rng(B), B, Cn)
    bufs = Bufs(dev)
    pack = run_pack(c, dev, bufs)
    f = run_fwd(c, dev, bufs, pack)
    d = {k: T(v, dev) if isinstance(v, np.ndarray) else v for k, v in lab.items()}

    def rider():
        out = dict(dwargs=bufs.out(B, 2 * (Cn - 1)), dhW=bufs.out(B, D))
        out['layer_grad'] = (bufs.out(D, 2 * (Cn - 1)), bufs.out(2 * (Cn - 1))) if layer_grad else None
        return out

    o1 = rider()
    rq = ops.ReduceQueue(dev) if defer else None
    r = run_bwd(c, dev, bufs, pack, f, defer=rq, label=dict(d, **o1))
    if rq is not None:
        rq.flush()
    r_now = run_bwd(c, dev, bufs, pack, f)          # immediate reduction, no rider
    o2 = rider()
    rq2 = ops.ReduceQueue(dev) if defer else None
    ops.vrnn_label_bwd(B, D, Cn, G4, r['dzsum_enc'], r['dzsum_dec'], d['Kenc_w'], d['Kdec_w'], d['wargs'], d['eps'], d['onehot'],
                       d['W'], d['hW'], d['Ka'], lab['prior'], lab['class_weight'], lab['w_kl_weight'], lab['inv_b'],
                       o2['dwargs'], o2['dhW'], layer_grad=o2['layer_grad'], ws=ops.Workspace(dev), defer=rq2)
    if rq2 is not None:
        rq2.flush()
    torch.cuda.synchronize()
    check_backward(c, f, r)
    for k in ('dz_dec', 'dz_enc', 'dzsum_dec', 'dzsum_enc', 'dzargs', 'dWz', 'dbz'):
        assert torch.equal(r[k], r_now[k]), k
    assert torch.equal(o1['dwargs'], o2['dwargs']) and torch.equal(o1['dhW'], o2['dhW'])
    want = PR.label_backward(N(r['dzsum_enc']), N(r['dzsum_dec']), *[lab[k] for k in ('Kenc_w', 'Kdec_w', 'wargs', 'eps',
                             'onehot', 'W', 'hW', 'Ka', 'prior', 'class_weight', 'w_kl_weight', 'inv_b')])
    np.testing.assert_allclose(N(o1['dwargs']), want['dwargs'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(N(o1['dhW']), want['dhW'], rtol=1e-4, atol=1e-5)
    if layer_grad:
        for a, b2, k in zip(o1['layer_grad'], o2['layer_grad'], ('dKa', 'dba')):
            assert torch.equal(a, b2), k
            np.testing.assert_allclose(N(a), want[k], rtol=1e-4, atol=1e-5, err_msg=k)
    bufs.check_canaries()


@pytest.mark.parametrize("L", [1, 5, 8])
def test_label_launch_writes_the_pair_pack(dev, L):
    """vrnn_label_fwd_x(pack=...): the weight pack the label launch writes as a by-product is clv_lstm_pair_pack's, bit for bit"""
    from clvae_amd import ops
    B, Tn, D, Cn = 2, 3, 88, 5
    rng = np.random.default_rng(L)
    c = make_case(1, 1, L, 'hard_sigmoid', True, 400 + L)
    bufs = Bufs(dev)
    want = run_pack(c, dev, bufs)
    got = bufs.out(ops.lstm_pair_pack_floats())
    lab = _label_inputs(rng, B, Cn)
    d = {k: T(v, dev) for k, v in lab.items() if isinstance(v, np.ndarray)}
    X = T((rng.random((B, Tn * D)) < 0.1).astype(np.float32), dev)
    Kh, bh = T(rng.standard_normal((Tn * D, D)) * 0.05, dev), T(rng.standard_normal(D) * 0.1, dev)
    ba = T(np.zeros(2 * (Cn - 1)), dev)
    z = lambda *sh: torch.empty(*sh, device=dev)
    ops.vrnn_label_fwd_x(B, D, Cn, G4, X, Tn * D, Tn * D, Kh, bh, z(B, D), d['Ka'], ba, d['eps'], d['onehot'], 0.2,
                         d['Kenc_w'], T(np.zeros(G4), dev), d['Kdec_w'], T(np.zeros(G4), dev), z(B, 2 * (Cn - 1)), z(B, Cn),
                         z(B, 3), z(B, G4), z(B, G4),
                         pack=(L, T(c['Ue'], dev), T(c['Ud'], dev), T(c['Kz'], dev), T(c['Wz'], dev), got))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    bufs.check_canaries()
