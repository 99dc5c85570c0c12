"""fp64 reference of the kernels that multiply piano-roll frames -- csrc/sparse_proj.hip (clv_sparse_proj, clv_sparse_proj2,
clv_sparse_dense, clv_sparse_outer) and csrc/outer_bf16.hip (clv_dense_outer_bf16, clv_dense_window_fwd_bf16) -- with
per-element bounds, the case tables that tests/test_window_reference.py (no GPU) and tests/test_gpu_window.py share, and an
fp32 evaluation of the same contracts in which summation orders can be chosen and faults planted.

Written from the contracts of include/clvae.h, not from the kernels' structure:

  sparse_proj       out[r,:N] = sum_k X[r,k] K[k,:]                                  X [R,ldx], K [nx,N]
  sparse_proj2      two of them over the same R frames
  sparse_dense      out[r,:N] = act(sum_j X[r,j] K[j,:] + bias), act none / relu
  sparse_outer      out[j,:N] = sum_b X[b,j] G[b,:];  colsum[c] = sum_b G[b,c];  gdot[c] = sum_b (H[b,c] - hb[c]) G[b,c]
  dense_outer_bf16  the same three outputs for frames that are exact in bf16
  dense_window_fwd_bf16   part[c][b][:N] = sum over the inputs i of chunk c of X[b,i] K[i,:]; `sum` is what the consumer
                    forms of them (here in fp64)

An input dict holds the arrays AS THEY LIE IN MEMORY: X [rows, ldx] with its padding columns (7.0, or 255 in byte frames),
G [Bn, ldg], H [Bn, ldh], the window's K [nx, ldk]; the references read the used columns only.  Frames of kind 'notes' and
'bytes' are uint8 arrays (the float launches get their float copy), 'dense' ones fp32-representable float64.  Inputs are
rounded to fp32 first; every ref_* function returns {output: (want, bound, flags)}; no output here needs flags.

bounds      U = 2^-24, BOUND_K = 32 (label_reference.py, pointwise_reference.py).  A dot product or sum gets
            BOUND_K U sum |terms|: out: sum |x k| over the inputs of the element (+ |bias|; the relu is 1-Lipschitz, so the
            bound goes through it unchanged); colsum: sum_b |G|; gdot: sum_b (|H| + |hb|) |G| (the subtraction rounds);
            a chunk's partial sum: the chunk's own magnitude; `sum`: the whole row's.  Where a case sums more than BOUND_K
            nonzero terms the honest fp32 evaluations of tests/test_window_reference.py (three orders, half of every bound to
            spare) are what justifies the constant.  No bound is taken from a GPU output.
exact       bound None, the 32 bits compared: sparse_proj / sparse_proj2 on 0/1 frames = the sequential fp32 sum of the
            listed kernel rows in ascending input index, from +0 (the header's order; fma(1, k, acc) is a plain add).  The GPU
            tests also hold bit for bit: a byte launch against the float launch of the same frames (every output), and
            sparse_proj2 against the two single launches.
            bound 0, equal as numbers: elements whose inputs are all zero (the bound formula gives 0 there by itself).
"""
import numpy as np

U = 2.0 ** -24
BOUND_K = 32
DENSITY = 0.0443
PAD_F, PAD_U8 = 7.0, 255
ACT_NONE, ACT_RELU = 0, 1          # CLV_ACT_* of include/clvae.h (asserted against _lib by the tests)
f32, f64 = np.float32, np.float64
A = np.abs


def _b(*terms):
    return BOUND_K * U * sum(terms)


def r32(a):
    return None if a is None else np.asarray(a, f32).astype(f64)


def used(X, n):
    """the n used columns of an array as it lies in memory, as fp64 of its fp32 (or byte) values"""
    return r32(np.asarray(X)[:, :n])


# ------------------------------------------------------------------------------------------------------------ checker --
def check(name, got, want, bound, flags=None):
    """every element of got within its bound of want.  Returns the worst error / bound ratio (0 where got = want); raises
    naming the worst element's index and its error as a multiple of its bound."""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    bound = np.broadcast_to(np.asarray(bound, f64), want.shape)
    err = A(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isfinite(got), np.nan_to_num(ratio, nan=np.inf), np.inf)
    bad = np.argwhere(ratio > 1.0)
    if bad.size:
        i = tuple(int(x) for x in bad[np.argmax(ratio[tuple(bad.T)])])
        raise AssertionError("%s%s: got %.9g, expected %.9g, error %.3g = %.3g x its bound %.3g (%d of %d elements off)"
                             % (name, list(i), got[i], want[i], err[i], ratio[i], bound[i], len(bad), want.size))
    return float(ratio.max()) if ratio.size else 0.0


def check_bits(name, got, want):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s%s: got %r, expected %r bit for bit (%d of %d elements off)"
                             % (name, list(i), got[i], want[i], len(bad), want.size))
    return 0.0


def check_all(name, got, ref):
    """{output: array} against {output: (want, bound, flags)}; bound None: bit for bit.  Returns {output: ratio}."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    return {k: check_bits(name + ' ' + k, got[k], ref[k][0]) if ref[k][1] is None
            else check(name + ' ' + k, got[k], *ref[k]) for k in sorted(ref)}


# --------------------------------------------------------------------------------------------------------- references --
def is_binary(X, nx):
    return bool(np.isin(np.asarray(X)[:, :nx], (0, 1)).all())


def _listed_rows_sum(x, K):
    """the sequential fp32 sum, from +0, of the rows K[k] with x[r,k] = 1, in ascending k"""
    K = np.asarray(K, f32)
    acc = np.zeros((x.shape[0], K.shape[1]), f32)
    for k in range(x.shape[1]):
        on = x[:, k] == 1
        if on.any():
            acc[on] = acc[on] + K[k]
    return acc


def ref_sparse_proj(X, nx, N, K, exact=True, **_):
    x, k = used(X, nx), r32(K)
    if exact and is_binary(X, nx):
        return dict(out=(_listed_rows_sum(x, k), None, None))
    return dict(out=(x @ k, _b(A(x) @ A(k)), None))


def ref_sparse_proj2(sets, N, exact=True, **_):
    return {'out%d' % i: ref_sparse_proj(s['X'], s['nx'], N, s['K'], exact)['out'] for i, s in enumerate(sets)}


def ref_sparse_dense(X, nx, N, K, bias, act, **_):
    x, k = used(X, nx), r32(K)
    pre, mag = x @ k, A(x) @ A(k)
    if bias is not None:
        pre, mag = pre + r32(bias), mag + A(r32(bias))
    return dict(out=(np.maximum(pre, 0.0) if act == ACT_RELU else pre, _b(mag), None))


def ref_outer(X, nx, N, G, colsum=False, H=None, hb=None, **_):
    """sparse_outer and dense_outer_bf16: one contract.  gdot is asked for by handing in H (and hb)."""
    x, g = used(X, nx), used(G, N)
    out = dict(out=(x.T @ g, _b(A(x).T @ A(g)), None))
    if colsum:
        out['colsum'] = (g.sum(0), _b(A(g).sum(0)), None)
    if H is not None:
        h, b = used(H, N), r32(hb)
        out['gdot'] = (((h - b) * g).sum(0), _b(((A(h) + A(b)) * A(g)).sum(0)), None)
    return out


ref_sparse_outer = ref_dense_outer_bf16 = ref_outer


def window_split(Bn, nx):
    """(splits, chunk) by the rule of include/clvae.h"""
    rb = -(-Bn // 64)
    chunks = max(1, min(-(-256 // rb), nx // 64))
    chunk = -(-(-(-nx // chunks)) // 32) * 32
    return -(-nx // chunk), chunk


def window_outputs(part):
    """what a launch leaves ([splits, Bn, N] fp32) and what its consumer forms of it (here in fp64)"""
    return dict(part=np.asarray(part, f32), sum=np.asarray(part, f64).sum(0))


def ref_dense_window_fwd_bf16(X, nx, N, K, **_):
    x, k = used(X, nx), used(K, N)
    splits, chunk = window_split(x.shape[0], nx)
    want, bound = np.zeros((splits,) + (x.shape[0], N)), np.zeros((splits,) + (x.shape[0], N))
    for c in range(splits):
        sl = slice(c * chunk, min(nx, (c + 1) * chunk))
        want[c], bound[c] = x[:, sl] @ k[sl], _b(A(x[:, sl]) @ A(k[sl]))
    return dict(part=(want, bound, None), sum=(x @ k, _b(A(x) @ A(k)), None))


REF = dict(sparse_proj=ref_sparse_proj, sparse_proj2=ref_sparse_proj2, sparse_dense=ref_sparse_dense,
           sparse_outer=ref_sparse_outer, dense_outer_bf16=ref_dense_outer_bf16, dense_window_fwd_bf16=ref_dense_window_fwd_bf16)


# ---------------------------------------------------------------------------------------------- fp32 building blocks --
ORDERS = ('forward', 'reversed', 'split')


def acc32(n, term, shape, order='forward', group=None):
    """the fp32 sum of term(0) .. term(n - 1) (fp32 arrays of `shape`) from +0: sequential 'forward' or 'reversed', or
    'split': a sequential partial sum per group(i), the partial sums added in ascending group"""
    idx = range(n - 1, -1, -1) if order == 'reversed' else range(n)
    if order == 'split':
        parts = {}
        for i in idx:
            g = group(i)
            parts[g] = parts.get(g, np.zeros(shape, f32)) + term(i)
        tot = np.zeros(shape, f32)
        for g in sorted(parts):
            tot = tot + parts[g]
        return tot
    assert order in ('forward', 'reversed'), order
    tot = np.zeros(shape, f32)
    for i in idx:
        tot = tot + term(i)
    return tot


def bf16(a):
    """fp32 -> the nearest bf16 number (ties to even), as fp32"""
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(f32)


def two_pieces(a):
    """an fp32 number without the last of its three bf16 pieces"""
    a = np.asarray(a, f32)
    p0 = bf16(a)
    return p0 + bf16(a - p0)


def seven_bits(a):
    """cut to 7 significant bits: one fewer than bf16 holds, so 0 / 1 survive and odd bytes from 129 on do not"""
    return (np.ascontiguousarray(a, f32).view(np.uint32) & np.uint32(0xfffe0000)).view(f32)


def _drop_nonzero(x, which, width=None):
    """x [rows, n] without the last ('last') or the fifth ('fifth') nonzero of every row -- of every `width` columns"""
    x = x.copy()
    n = x.shape[1]
    for c0 in range(0, n, width or n):
        blk = x[:, c0:c0 + (width or n)]
        nz = blk != 0
        cnt = np.cumsum(nz, 1)
        hit = nz & (cnt == (cnt[:, -1:] if which == 'last' else 5))
        blk[hit] = 0
    return x


# faults of the way X is read, shared by the kernels (inputs along axis 1 of X)
F_LAST, F_LASTCH, F_FIFTH = 'last nonzero of a row dropped', 'last nonzero of a chunk dropped', 'fifth nonzero of a chunk dropped'
F_IN_LAST, F_IN64, F_IN65 = 'input nx-1 ignored', 'input 64 ignored', 'input 65 ignored'
F_PAD, F_LDX = 'a padding column of X read', 'ldx taken as nx'
F_XBF16, F_X7 = 'X rounded to bf16', 'X cut to 7 significant bits'
F_ROW, F_COL_LAST, F_COL64 = 'last row dropped', 'column N-1 not written', 'column 64 not written'
F_LDG, F_LDH, F_LDK = 'ldg taken as N', 'ldh taken as N', 'ldk taken as N'
F_CLAMP, F_HB, F_GLOW, F_KLOW = 'a row beyond Bn added once more', 'hbias not subtracted', 'lowest bf16 piece of G dropped', \
    'lowest bf16 piece of K dropped'
F_NOBIAS, F_NX2 = 'no relu where bias is NULL', "second projection with the first one's nx"
F_TWICE, F_NONE = 'chunk border a stage late: inputs counted twice', 'chunk border a stage early: inputs counted in none'


def _restride(M, n):
    """the matrix a kernel sees that takes the leading dimension of M [rows, ld] for n"""
    M = np.asarray(M)
    return M.reshape(-1)[:M.shape[0] * n].reshape(M.shape[0], n)


def _frames32(X, nx, fault):
    """(x [rows, inputs] fp32, kernel row of every input) as a kernel with `fault` reads X"""
    X = np.asarray(X)
    x = (_restride(X, nx) if fault == F_LDX else X[:, :nx + 1] if fault == F_PAD and X.shape[1] > nx else X[:, :nx]).astype(f32)
    krow = np.minimum(np.arange(x.shape[1]), nx - 1)
    if fault == F_LAST:
        x = _drop_nonzero(x, 'last')
    if fault in (F_LASTCH, F_FIFTH):
        x = _drop_nonzero(x, 'last' if fault == F_LASTCH else 'fifth', 64)
    for f, k in ((F_IN_LAST, nx - 1), (F_IN64, 64), (F_IN65, 65)):
        if fault == f and k < nx:
            x[:, k] = 0
    if fault == F_XBF16:
        x = bf16(x)
    if fault == F_X7:
        x = seven_bits(x)
    return x, krow


def _unwritten(out, fault, N):
    out = np.array(out, f32)
    if fault == F_ROW:
        out[-1] = np.nan
    if fault == F_COL_LAST:
        out[..., N - 1] = np.nan
    if fault == F_COL64 and N > 64:
        out[..., 64] = np.nan
    return out


def f32_sparse_proj(X, nx, N, K, order='forward', fault=None, **_):
    x, krow = _frames32(X, nx, fault)
    K = np.asarray(K, f32)
    out = acc32(x.shape[1], lambda i: x[:, i:i + 1] * K[krow[i]], (x.shape[0], N), order, lambda i: i // 64)
    return dict(out=_unwritten(out, fault, N))


def f32_sparse_proj2(sets, N, order='forward', fault=None, **_):
    out = {}
    for i, s in enumerate(sets):
        nx = s['nx']
        if fault == F_NX2 and i == 1:          # as many inputs as the first projection has (on into the padding and the next
            X1, n0 = np.asarray(s['X']), sets[0]['nx']                       # frame); kernel rows beyond its own clamped
            at = np.arange(X1.shape[0])[:, None] * X1.shape[1] + np.arange(n0)[None, :]
            x = X1.reshape(-1)[np.minimum(at, X1.size - 1)].astype(f32)
            K = np.asarray(s['K'], f32)[np.minimum(np.arange(n0), nx - 1)]
            out['out1'] = acc32(n0, lambda j: x[:, j:j + 1] * K[j], (x.shape[0], N), order, lambda j: j // 64)
        else:
            out['out%d' % i] = f32_sparse_proj(s['X'], nx, N, s['K'], order, None if fault == F_NX2 else fault)['out']
    return out


def f32_sparse_dense(X, nx, N, K, bias, act, order='forward', fault=None, **_):
    x, krow = _frames32(X, nx, fault)
    K = np.asarray(K, f32)
    out = acc32(x.shape[1], lambda i: x[:, i:i + 1] * K[krow[i]], (x.shape[0], N), order, lambda i: (i // 64) % 16)
    if bias is not None:
        out = out + np.asarray(bias, f32)
    if act == ACT_RELU and not (fault == F_NOBIAS and bias is None):
        out = np.maximum(out, f32(0))
    return dict(out=_unwritten(out, fault, N))


def f32_outer(X, nx, N, G, colsum=False, H=None, hb=None, order='forward', fault=None, **_):
    x, _ = _frames32(np.asarray(X), nx, None if fault in (F_LAST, F_PAD) else fault)
    x = x[:, :nx]
    if fault == F_LAST:                          # the last nonzero batch row of every input
        x = _drop_nonzero(x.T, 'last').T
    g = (_restride(G, N) if fault == F_LDG else np.asarray(G)[:, :N]).astype(f32)
    gp = two_pieces(g) if fault == F_GLOW else g
    Bn = x.shape[0]
    rows = Bn - 1 if fault == F_ROW else Bn
    stage = lambda b: b // 32
    out = dict(out=acc32(rows, lambda b: x[b][:, None] * gp[b][None, :], (nx, N), order, stage))
    if fault == F_COL_LAST:
        out['out'][:, N - 1] = np.nan
    if fault == F_COL64 and N > 64:
        out['out'][:, 64] = np.nan
    again = [Bn - 1] if fault == F_CLAMP else []            # the clamped row of a round that the batch does not fill
    if colsum:
        out['colsum'] = acc32(rows, lambda b: g[b], (N,), order, stage)
        for b in again:
            out['colsum'] = out['colsum'] + g[b]
    if H is not None:
        h = (_restride(H, N) if fault == F_LDH else np.asarray(H)[:, :N]).astype(f32)
        b32 = np.zeros(N, f32) if fault == F_HB else np.asarray(hb, f32)
        out['gdot'] = acc32(rows, lambda b: (h[b] - b32) * g[b], (N,), order, stage)
        for b in again:
            out['gdot'] = out['gdot'] + (h[b] - b32) * g[b]
    return out


f32_sparse_outer = f32_dense_outer_bf16 = f32_outer


def f32_dense_window_fwd_bf16(X, nx, N, K, order='forward', fault=None, **_):
    x, _ = _frames32(X, nx, fault)
    k = (_restride(K, N) if fault == F_LDK else np.asarray(K)[:, :N]).astype(f32)
    if fault == F_KLOW:
        k = two_pieces(k)
    Bn = x.shape[0]
    splits, chunk = window_split(Bn, nx)
    part = np.zeros((splits, Bn, N), f32)
    for c in range(splits):
        i0, i1 = c * chunk, min(nx, (c + 1) * chunk)
        if c + 1 < splits:
            i1 += 32 if fault == F_TWICE else -32 if fault == F_NONE else 0
        i1 = min(i1, nx)
        part[c] = acc32(i1 - i0, lambda i: x[:, i0 + i:i0 + i + 1] * k[i0 + i], (Bn, N), order, lambda i: i // 32)
    if fault == F_ROW:
        part[:, -1] = np.nan
    if fault == F_COL_LAST:
        part[..., N - 1] = np.nan
    return window_outputs(part)


F32 = dict(sparse_proj=f32_sparse_proj, sparse_proj2=f32_sparse_proj2, sparse_dense=f32_sparse_dense,
           sparse_outer=f32_sparse_outer, dense_outer_bf16=f32_dense_outer_bf16, dense_window_fwd_bf16=f32_dense_window_fwd_bf16)

# ------------------------------------------------------------------------------------------------------- planted faults --
# FAULTS[kernel][fault] = which cases must reject it (a predicate of the case; at least one case satisfies it), or None: no
# case may notice -- rounding X to bf16 is what the two bf16 kernels do, and every uint8 value is a bf16 number; it takes one
# bit fewer (F_X7) to show on byte frames, and 0 / 1 frames survive that too.
_padx = lambda c: c['ldx'] > c['nx'] and c['R'] > 1
_many = lambda c: c['R'] >= 15
FAULTS = dict(
    sparse_proj={
        F_LAST: _many,
        F_IN_LAST: lambda c: c['R'] >= 15 and c['kind'] != 'notes',
        F_IN64: lambda c: c['nx'] > 64 and c['kind'] != 'notes' and c['R'] >= 15,
        F_IN65: lambda c: c['nx'] > 65 and c['kind'] != 'notes' and c['R'] >= 15,
        F_PAD: lambda c: c['ldx'] > c['nx'],
        F_LDX: _padx,
        F_XBF16: lambda c: c['kind'] == 'dense' and c['R'] >= 15,
        F_X7: lambda c: c['kind'] == 'bytes',
        F_ROW: lambda c: True,
        F_COL_LAST: lambda c: True,
        F_COL64: lambda c: c['N'] > 64},
    sparse_proj2={
        F_NX2: lambda c: c['sets'][0][0] != c['sets'][1][0],
        F_LDX: lambda c: any(ldx > nx for nx, ldx in c['sets']),
        F_ROW: lambda c: True},
    sparse_dense={
        F_LASTCH: lambda c: c['hand'],
        F_FIFTH: lambda c: c['hand'],
        F_IN_LAST: lambda c: c['kind'] == 'dense' and c['R'] > 1,
        F_IN64: lambda c: c['hand'],
        F_IN65: lambda c: c['hand'],
        F_PAD: lambda c: c['ldx'] > c['nx'],
        F_LDX: _padx,
        F_XBF16: lambda c: c['kind'] == 'dense' and c['R'] > 1,
        F_NOBIAS: lambda c: not c['bias'] and c['act'] == ACT_RELU,
        F_ROW: lambda c: True,
        F_COL_LAST: lambda c: True,
        F_COL64: lambda c: c['N'] > 64},
    sparse_outer={
        F_LAST: lambda c: c['Bn'] > 1,
        F_IN_LAST: lambda c: c['kind'] == 'dense' and c['Bn'] > 1,
        F_IN64: lambda c: c['nx'] > 64 and c['kind'] == 'dense' and c['Bn'] > 1,
        F_IN65: lambda c: c['nx'] > 65 and c['kind'] == 'dense' and c['Bn'] > 1,
        F_LDX: lambda c: c['ldx'] > c['nx'] and c['Bn'] > 1,
        F_LDG: lambda c: c['ldg'] > c['N'] and c['Bn'] > 1,
        F_LDH: lambda c: c['gdot'] and c['ldh'] > c['N'] and c['Bn'] > 1,
        F_ROW: lambda c: c['Bn'] > 1 and (c['colsum'] or c['gdot']),
        F_CLAMP: lambda c: c['colsum'] or c['gdot'],
        F_HB: lambda c: c['gdot'],
        F_XBF16: lambda c: c['kind'] == 'dense' and c['Bn'] > 1,
        F_COL_LAST: lambda c: True,
        F_COL64: lambda c: c['N'] > 64},
    dense_outer_bf16={
        F_LAST: lambda c: c['Bn'] > 1,
        F_IN_LAST: lambda c: c['kind'] == 'bytes',
        F_IN64: lambda c: c['nx'] > 64 and c['kind'] == 'bytes',
        F_IN65: lambda c: c['nx'] > 65 and c['kind'] == 'bytes',
        F_LDX: lambda c: c['ldx'] > c['nx'] and c['Bn'] > 1,
        F_LDG: lambda c: c['ldg'] > c['N'] and c['Bn'] > 1,
        F_LDH: lambda c: c['gdot'] and c['ldh'] > c['N'] and c['Bn'] > 1,
        F_ROW: lambda c: c['Bn'] > 1 and (c['colsum'] or c['gdot']),
        F_CLAMP: lambda c: c['colsum'] or c['gdot'],
        F_HB: lambda c: c['gdot'],
        # the third piece is up to 2^-17 |g|, a third of the time more than the 2^-19 |x g| that one term is allowed: it shows
        # where an element sums two or three terms and the case has more than a row's handful of G values
        F_GLOW: lambda c: c['Bn'] in (2, 3),
        F_XBF16: None,
        F_X7: lambda c: c['kind'] == 'bytes',
        F_COL_LAST: lambda c: True,
        F_COL64: lambda c: c['N'] > 64},
    dense_window_fwd_bf16={
        F_IN_LAST: lambda c: c['kind'] == 'bytes',
        F_IN64: lambda c: c['nx'] > 64 and c['kind'] == 'bytes',
        F_LDX: lambda c: c['ldx'] > c['nx'] and c['Bn'] > 1,
        F_LDK: lambda c: c['ldk'] > c['N'] and c['nx'] > 8,
        F_KLOW: lambda c: c['kind'] == 'notes' and c['Bn'] >= 15,
        F_XBF16: None,
        F_X7: lambda c: c['kind'] == 'bytes',
        F_TWICE: lambda c: window_split(c['Bn'], c['nx'])[0] > 1 and c['kind'] == 'bytes',
        F_NONE: lambda c: window_split(c['Bn'], c['nx'])[0] > 1 and c['kind'] == 'bytes',
        F_ROW: lambda c: True,
        F_COL_LAST: lambda c: True})
# ... and which cases must NOT notice: a fault that changes nothing for them (0 / 1 are exact in every format here)
HARMLESS = {F_XBF16: lambda c: c.get('kind') in ('notes', 'bytes'), F_X7: lambda c: c.get('kind') == 'notes'}


# -------------------------------------------------------------------------------------------------------- case tables --
# The smallest shapes at which each path can still go wrong; test_window_reference.py asserts the edges they are there for.
def _cases(keys, rows, seed):
    return [dict(zip(keys, r), seed=seed + i) for i, r in enumerate(rows)]


CASES = dict(
    # (100, 384) is exactly the 150 KB of LDS; R 4095 / 4096 / 4097: the row split below, at and over the cap of 256
    sparse_proj=_cases(('R', 'nx', 'N', 'ldx', 'ldo', 'kind'), [
        (4097, 88, 352, 88, 352, 'notes'),
        (4096, 16, 64, 20, 68, 'bytes'),
        (4095, 4, 1, 4, 3, 'dense'),
        (1, 1, 4, 3, 4, 'dense'),
        (15, 64, 64, 64, 72, 'notes'),
        (16, 65, 64, 68, 64, 'bytes'),
        (17, 128, 300, 128, 304, 'notes'),
        (17, 100, 384, 104, 384, 'dense'),
        (16, 4, 63, 8, 63, 'dense'),
        (15, 4, 65, 4, 70, 'bytes'),
        (33, 90, 352, 92, 356, 'dense'),
        (17, 88, 352, 92, 352, 'bytes'),
        (7, 88, 352, 92, 356, 'notes')], 1000),
    # sets: (nx, ldx) of the two projections; the cap is 128 workgroups per projection
    sparse_proj2=_cases(('R', 'N', 'ldo', 'sets', 'kind'), [
        (2047, 352, 352, ((88, 88), (70, 92)), 'notes'),
        (2048, 64, 68, ((16, 20), (64, 64)), 'bytes'),
        (2049, 64, 64, ((65, 68), (4, 4)), 'dense'),
        (17, 384, 388, ((88, 92), (100, 100)), 'notes'),
        (16, 64, 64, ((128, 128), (65, 72)), 'bytes')], 1100),
    # hand: row r's first 64-input chunk holds exactly 0, 1, 3, 4, 5 nonzeros (r = 0 .. 4), its second one 64
    sparse_dense=_cases(('R', 'nx', 'N', 'ldx', 'ldo', 'bias', 'act', 'kind', 'hand'), [
        (5, 11264, 88, 11268, 88, True, ACT_RELU, 'notes', False),
        (1, 1, 2, 3, 2, False, ACT_NONE, 'dense', False),
        (5, 63, 18, 63, 20, True, ACT_RELU, 'dense', False),
        (5, 64, 128, 68, 128, False, ACT_RELU, 'dense', False),
        (5, 65, 2, 65, 5, True, ACT_NONE, 'dense', False),
        (5, 200, 18, 203, 18, False, ACT_NONE, 'dense', True),
        (5, 1024, 88, 1024, 90, True, ACT_RELU, 'notes', False),
        (5, 1030, 128, 1032, 132, False, ACT_RELU, 'dense', True),
        (1, 1030, 88, 1030, 88, True, ACT_NONE, 'notes', False),
        (5, 200, 18, 200, 18, True, ACT_RELU, 'notes', True),
        (3, 200, 18, 200, 18, True, ACT_NONE, 'dense', False),
        (2, 64, 128, 64, 128, True, ACT_RELU, 'dense', False)], 1200),
    # chain: H = relu(X K + hb) and G masked by H > 0, as in a training step
    sparse_outer=_cases(('Bn', 'nx', 'N', 'ldx', 'ldg', 'ldo', 'ldh', 'colsum', 'gdot', 'kind', 'chain'), [
        (1, 1, 2, 1, 2, 2, 2, False, False, 'dense', False),
        (127, 63, 18, 65, 20, 19, 22, True, True, 'notes', False),
        (128, 64, 88, 64, 90, 88, 88, True, False, 'dense', False),
        (129, 65, 128, 68, 128, 130, 130, False, True, 'notes', False),
        (257, 130, 88, 131, 92, 90, 90, True, True, 'notes', True),
        (257, 64, 2, 67, 4, 3, 2, False, False, 'dense', False),
        (129, 130, 18, 130, 18, 18, 20, True, True, 'dense', True),
        (1, 65, 18, 66, 20, 18, 18, True, True, 'dense', False),
        (100, 130, 88, 130, 88, 88, 88, True, False, 'notes', False),
        (300, 70, 18, 70, 18, 18, 18, True, False, 'dense', False)], 1300),
    # nx 9504: 99 tiles of 96, the 3-wave kernel; 9508 and 9600: the 6-wave kernel with a ragged and a full last tile
    dense_outer_bf16=_cases(('Bn', 'nx', 'N', 'ldx', 'ldg', 'ldo', 'ldh', 'colsum', 'gdot', 'kind'), [
        (1, 4, 4, 8, 8, 6, 4, False, False, 'bytes'),
        (31, 44, 20, 48, 24, 22, 22, True, False, 'notes'),
        (32, 48, 92, 52, 96, 92, 94, False, True, 'bytes'),
        (33, 52, 96, 52, 100, 100, 96, True, True, 'notes'),
        (96, 100, 20, 104, 20, 23, 26, True, True, 'bytes'),
        (128, 48, 4, 48, 8, 4, 4, True, False, 'notes'),
        (129, 100, 92, 108, 96, 95, 96, False, True, 'bytes'),
        (161, 52, 96, 56, 104, 96, 98, True, True, 'notes'),
        (33, 9504, 20, 9508, 24, 20, 20, True, True, 'notes'),
        (25, 9508, 96, 9512, 100, 98, 98, True, True, 'bytes'),
        (33, 9600, 92, 9604, 92, 94, 92, True, True, 'notes'),
        (2, 44, 4, 44, 4, 4, 6, False, True, 'bytes'),
        (3, 100, 20, 100, 24, 20, 20, True, False, 'bytes'),
        (7, 4, 92, 12, 92, 92, 92, True, True, 'bytes'),
        (25, 48, 96, 52, 100, 97, 98, True, True, 'bytes'),
        (49, 52, 20, 52, 20, 20, 20, True, True, 'notes')], 1400),
    # (17, 120) and (4100, 520) are there for 4 and 5 stages per chunk, which the other sizes cannot reach
    dense_window_fwd_bf16=_cases(('Bn', 'nx', 'N', 'ldx', 'ldk', 'kind'), [
        (1, 8, 4, 12, 8, 'bytes'),
        (15, 32, 20, 32, 24, 'notes'),
        (16, 40, 92, 44, 92, 'bytes'),
        (17, 64, 96, 68, 100, 'notes'),
        (63, 128, 20, 132, 20, 'bytes'),
        (64, 136, 92, 136, 96, 'notes'),
        (65, 200, 96, 204, 96, 'bytes'),
        (130, 520, 4, 524, 8, 'notes'),
        (17, 2000, 92, 2004, 96, 'bytes'),
        (17, 120, 20, 124, 24, 'bytes'),
        (4100, 520, 4, 520, 4, 'notes'),
        (37, 96, 20, 96, 20, 'notes')], 1500))

HAND_COUNTS = (0, 1, 3, 4, 5)


def frames(rng, rows, nx, ldx, kind):
    """[rows, ldx] as it lies in memory: uint8 for 'notes' (0 / 1 at the data's density) and 'bytes' (any value), float64 for
    'dense' (normal, with exact zeros and some -0.0); row 0 all zero and row 1 all ones where there are three rows; the
    padding columns hold a large value"""
    if kind == 'dense':
        x = r32(rng.standard_normal((rows, nx)))
        x[rng.random((rows, nx)) < 0.15] = 0.0
        x[rng.random((rows, nx)) < 0.05] = -0.0
        X = np.full((rows, ldx), PAD_F)
    else:
        x = (rng.random((rows, nx)) < DENSITY).astype(np.uint8) if kind == 'notes' else rng.integers(0, 256, (rows, nx)).astype(np.uint8)
        X = np.full((rows, ldx), PAD_U8, np.uint8)
    if rows >= 3:
        x[0], x[1] = 0, 1
    X[:, :nx] = x
    return X


def scaled(rng, rows, cols, ld=None, scale=1.0):
    """normal, every row scaled by exp(normal) so that low bf16 pieces matter; [rows, ld] with 7.0 in the padding columns"""
    M = np.full((rows, ld or cols), PAD_F)
    M[:, :cols] = r32(rng.standard_normal((rows, cols)) * np.exp(rng.standard_normal((rows, 1))) * scale)
    return M


def proj_inputs(c):
    rng = np.random.default_rng(c['seed'])
    return dict(X=frames(rng, c['R'], c['nx'], c['ldx'], c['kind']), nx=c['nx'], N=c['N'], K=scaled(rng, c['nx'], c['N']))


def proj2_inputs(c):
    rng = np.random.default_rng(c['seed'])
    return dict(N=c['N'], sets=[dict(X=frames(rng, c['R'], nx, ldx, c['kind']), nx=nx, K=scaled(rng, nx, c['N']))
                                for nx, ldx in c['sets']])


def dense_inputs(c):
    rng = np.random.default_rng(c['seed'])
    R, nx = c['R'], c['nx']
    X = frames(rng, R, nx, c['ldx'], c['kind'])
    if c['hand']:
        for r, cnt in enumerate(HAND_COUNTS):
            v = rng.standard_normal(64 + cnt)
            v[v == 0] = 1.0
            if c['kind'] != 'dense':
                v[:] = 1
            X[r, :64] = 0
            X[r, rng.permutation(64)[:cnt]] = r32(v[:cnt])
            X[r, 64:128] = r32(v[cnt:])
    return dict(X=X, nx=nx, N=c['N'], K=scaled(rng, nx, c['N'], scale=0.1), bias=r32(rng.standard_normal(c['N'])) if c['bias'] else None,
                act=c['act'])


def outer_inputs(c):
    rng = np.random.default_rng(c['seed'])
    Bn, nx, N = c['Bn'], c['nx'], c['N']
    X = frames(rng, Bn, nx, c['ldx'], c['kind'])
    if nx > 3 and c['seed'] % 2 == 0:            # (the other cases keep their all-ones row whole)
        X[:, 2] = 0                              # an input that no batch row has: its row of the gradient is zero, exactly
    G = scaled(rng, Bn, N, c['ldg'])
    d = dict(X=X, nx=nx, N=N, G=G, colsum=c['colsum'])
    if c['gdot']:
        hb = r32(rng.standard_normal(N))
        H = np.full((Bn, c['ldh']), PAD_F)
        if c.get('chain'):
            K = scaled(rng, nx, N, scale=0.3)
            H[:, :N] = r32(np.maximum(used(X, nx) @ K + hb, 0.0))
            G[:, :N] *= H[:, :N] > 0
            d['K'] = K
        else:
            H[:, :N] = r32(np.maximum(rng.standard_normal((Bn, N)), 0.0))
        d.update(H=H, hb=hb)
    return d


def window_inputs(c):
    rng = np.random.default_rng(c['seed'])
    return dict(X=frames(rng, c['Bn'], c['nx'], c['ldx'], c['kind']), nx=c['nx'], N=c['N'], K=scaled(rng, c['nx'], c['N'], c['ldk']))


INPUTS = dict(sparse_proj=proj_inputs, sparse_proj2=proj2_inputs, sparse_dense=dense_inputs, sparse_outer=outer_inputs,
              dense_outer_bf16=outer_inputs, dense_window_fwd_bf16=window_inputs)
BYTE_KERNELS = ('sparse_proj', 'sparse_proj2', 'dense_outer_bf16', 'dense_window_fwd_bf16')      # the entries with x_u8


def runs(kernels=None):
    """every (kernel, case, inputs) of the tables"""
    for k, cases in CASES.items():
        if kernels is None or k in kernels:
            for c in cases:
                yield k, c, INPUTS[k](c)


# what the launches do with a shape, restated from the kernels' launch rules for the coverage assertions
def proj_workgroups(R, nset):
    """(workgroups per projection, frames per workgroup, workgroups whose first frame is at or past R)"""
    cap = 256 // nset
    wgs = -(-R // 16) if R < cap * 16 else cap
    per = -(-R // wgs)
    return wgs, per, sum(1 for b in range(wgs) if b * per >= R)


def outer_waves(nx):
    """waves per workgroup of clv_dense_outer_bf16's own launch: 6 (96 inputs each) from 100 such tiles on, else 3 (48)"""
    return 6 if -(-nx // 96) >= 100 else 3


def window_stages(Bn, nx):
    """the stage counts of the chunks, and the inputs in every chunk's last stage"""
    splits, chunk = window_split(Bn, nx)
    n = [min(nx, (c + 1) * chunk) - c * chunk for c in range(splits)]
    return [-(-v // 32) for v in n], [(v - 1) % 32 + 1 for v in n], n
