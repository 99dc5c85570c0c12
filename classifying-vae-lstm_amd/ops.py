"""Thin torch-tensor wrappers over the C ABI (include/clvae.h).

torch is used for device memory and streams only; every computation below is a
HIP kernel of libclvae_hip.so.  All tensors must be contiguous float32 CUDA
tensors (views with a row stride are passed as (tensor, ld)).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_MASKPOS, check  # noqa: F401


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Workspace:
    """A growable byte buffer on the device handed to ops that need scratch."""

    def __init__(self, device, nbytes=1 << 20):
        self.device = device
        self.buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)

    def ensure(self, nbytes):
        if self.buf.numel() < nbytes:
            self.buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
        return self.buf


class ReduceQueue:
    """Pending split-K reductions of one backward pass (the `job` argument of the products + clv_splitk_reduce_multi).
    Every queued product keeps its partial slabs in its own scratch buffer until flush(); the buffers are
    kept per queue slot, so a step that queues the same products in the same order reuses the same memory
    (and a captured hipGraph sees fixed pointers)."""
    MAX_JOBS = 16

    def __init__(self, device):
        self.device = device
        self.jobs = (_lib.ReduceJob * self.MAX_JOBS)()
        self.slots = [None] * self.MAX_JOBS
        self.n = 0

    def scratch(self, nbytes):
        if self.n >= self.MAX_JOBS:
            raise _lib.ClvError("ReduceQueue: more than %d pending reductions" % self.MAX_JOBS)
        buf = self.slots[self.n]
        if buf is None or buf.numel() < nbytes:
            buf = self.slots[self.n] = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=self.device)
        return buf

    def next_job(self):
        """the next slot's job, as an address: an argument, or a job pointer that travels inside a struct"""
        j = C.c_void_p(C.addressof(self.jobs) + self.n * C.sizeof(_lib.ReduceJob))
        self.n += 1
        return j

    def flush(self, means=None, out=None, skinny=None, outer=None):
        """Run the pending reductions in one launch.  means: up to five (tensor, n, stride) terms whose means go to
        out[k] from extra blocks of the same launch (a step's loss terms: no launch of their own).  skinny: up to two
        dict(A, lda, rows, B, ldb, N, K, C, ldc, bias_row) few-row products A[:, :rows]^T B riding along as well.
        outer: the arguments of dense_outer_bf16 as a dict (Bn, nx, N, X, ldx, G, ldg, out and optionally ldo, colsum, gdot)
        -- that product as workgroups of the same launch (clv_splitk_reduce_multi_outer; reduce_outer_supported() says
        which shapes), every result bit for bit what the two launches give."""
        if means or skinny or self.n or outer is not None:
            means = means or []
            k = len(means)
            xs = (C.c_void_p * max(k, 1))(*[_ptr(t) for t, _, _ in means])
            ns = (C.c_int * max(k, 1))(*[int(n) for _, n, _ in means])
            st = (C.c_int * max(k, 1))(*[int(s) for _, _, s in means])
            skinny = skinny or []
            riders = (_lib.SkinnyProduct * max(len(skinny), 1))()
            for i, p in enumerate(skinny):
                riders[i] = _lib.SkinnyProduct(_ptr(p['A']), p['lda'], p['rows'], _ptr(p['B']), p['ldb'], p['N'], p['K'],
                                               _ptr(p['C']), p['ldc'], _ptr(p.get('bias_row')))
            args = (self.jobs, self.n, xs if k else None, ns if k else None, st if k else None, k,
                    _ptr(out) if k else None, riders if skinny else None, len(skinny))
            if outer is None:
                check(_lib.lib().clv_splitk_reduce_multi(*args, _stream()), "clv_splitk_reduce_multi")
            else:
                o = outer
                h, ldh, hb, go = o['gdot'] if o.get('gdot') is not None else (None, 0, None, None)
                ldo = o['ldo'] if o.get('ldo') is not None else o['N']
                check(_lib.lib().clv_splitk_reduce_multi_outer(
                    *args, o['Bn'], o['nx'], o['N'], _ptr(o['X']), _is_u8(o['X']), o['ldx'], _ptr(o['G']), o['ldg'], _ptr(o['out']),
                    ldo, _ptr(o.get('colsum')), _ptr(h), int(ldh), _ptr(hb), _ptr(go), _stream()), "clv_splitk_reduce_multi_outer")
        self.n = 0


def _scratch(need, ws, defer):
    """(buf, job) for a producer's slabs: the queue's next slot (its buffer first, then its job: the buffers are cached
    per slot) under a ReduceQueue, else the Workspace and no job -- the reduction then runs inside the call."""
    if defer is None:
        return ws.ensure(need), None
    return defer.scratch(need), defer.next_job()


def _scratch_regions(needs, ws, defer):
    """[(address, job)] for the slab regions of ONE call (need None: no such region, (None, None)): a queue slot each, in
    order, under a ReduceQueue; else one Workspace buffer, every region behind the 256-byte-aligned end of the one before."""
    if defer is not None:
        slots = [_scratch(n, None, defer) if n is not None else (None, None) for n in needs]
        return [(buf.data_ptr() if buf is not None else None, job) for buf, job in slots]
    offs, end = [], 0
    for n in needs:
        offs.append((end + 255) // 256 * 256)
        end = offs[-1] + (n or 0)
    if all(n is None for n in needs):
        return [(None, None)] * len(needs)
    base = _scratch(end, ws, None)[0].data_ptr()
    return [(base + o if n is not None else None, None) for n, o in zip(needs, offs)]


def reduce_outer_supported(Bn, nx, N, ldx, ldg):
    """shapes ReduceQueue.flush(outer=...) takes"""
    return bool(_lib.lib().clv_splitk_reduce_multi_outer_supported(Bn, nx, N, ldx, ldg))


def gemm(A, B, C_out, M, N, K, ta=False, tb=False, lda=None, ldb=None, ldc=None, alpha=1.0, beta=0.0,
         bias=None, act=ACT_NONE, aux=None, split_k=None, ws=None, defer=None):
    """C[M,N] = act(alpha*op(A).op(B) + bias + beta*C); A/B/C are tensors (possibly offset views).
    defer: a ReduceQueue -- a split product leaves its reduction (and epilogue) pending until defer.flush()."""
    L = _lib.lib()
    lda = lda if lda is not None else (M if ta else K)
    ldb = ldb if ldb is not None else (K if tb else N)
    ldc = ldc if ldc is not None else N
    if split_k is None:
        split_k = L.clv_gemm_auto_split(M, N, K)
    wsp, wsb, job = None, 0, None
    if split_k > 1:
        buf, job = _scratch(L.clv_gemm_workspace_bytes(M, N, split_k), ws, defer)
        wsp, wsb = _ptr(buf), buf.numel()
    check(L.clv_gemm_f32(int(ta), int(tb), M, N, K, float(alpha), _ptr(A), lda, _ptr(B), ldb, float(beta),
                                  _ptr(C_out), ldc, _ptr(bias), act, _ptr(aux), split_k, wsp, wsb, job, _stream()),
          "clv_gemm_f32")


def _prob_array(probs, N):
    arr = (_lib.GemmProb * len(probs))()
    for i, p in enumerate(probs):
        A = p.get('A')
        arr[i] = _lib.GemmProb(A.data_ptr() if A is not None else None, p.get('lda', p['M']), p['M'],
                               p['C'].data_ptr(), p.get('ldc', N), p.get('shift', 0), p.get('zero_period', 0),
                               int(p.get('ones', 0)))
    return arr


def gemm_grouped_tn(probs, N, K, B, ws, ldb=None, beta=0.0, split_k=None, defer=None, split_scale=1):
    """probs: list of dict(A=tensor|None, lda, M, C=tensor, ldc, shift=0, zero_period=0, ones=0|1|2);
    ones=1: implicit row of ones (M == 1); ones=2: row M-1 is an implicit row of ones appended to A's M-1 columns;
    C_p[M_p,N] = A_p^T . B for every problem in one launch (all share B [K,N])."""
    L = _lib.lib()
    arr, n = _prob_array(probs, N), len(probs)
    if split_k is None:
        split_k = L.clv_gemm_grouped_auto_split(arr, n, N, K)
        if split_k > 1:
            split_k *= int(split_scale)      # finer grid: more, shorter workgroups (see VrnnEngine.fine_grid)
    wsp, wsb, job = None, 0, None
    if split_k > 1:
        buf, job = _scratch(L.clv_gemm_grouped_workspace_bytes(arr, n, N, split_k), ws, defer)
        wsp, wsb = _ptr(buf), buf.numel()
    check(L.clv_gemm_grouped_tn(arr, n, N, K, _ptr(B), ldb if ldb is not None else N, float(beta), split_k,
                                         wsp, wsb, job, _stream()), "clv_gemm_grouped_tn")


def lstm_wgrad_supported(N, nx, nh, nz, x_exact_bf16):
    return bool(_lib.lib().clv_lstm_wgrad_supported(N, nx, nh, nz, int(bool(x_exact_bf16))))


def lstm_wgrad_rows_supported(K, N, X, ldx, x_exact_bf16, ldh, ldz, nz):
    """Do K rows of these strides stay inside the kernel's 32-bit offsets (every operand below 2 GiB: include/clvae.h)?"""
    return bool(_lib.lib().clv_lstm_wgrad_rows_supported(K, ldx, _frames_mode(X, x_exact_bf16), ldh, ldz, nz, N))


def lstm_wgrad(K, N, X, ldx, nx, x_exact_bf16, H, ldh, nh, T, Z, ldz, nz, dz, dKx, dU, dKz, ws, defer=None, beta=0.0,
               split_scale=1):
    """All kernel gradients of one LSTM in one pass over dz (split-bf16 products, 6 of the 9 piece pairs: fp32-rounding
    accuracy; csrc/wgrad_bf16.hip):
    dKx = X^T dz, dU = H'^T dz (H' = hs shifted by one step, zero at window starts: period T), dKz = Z^T dz.
    split_scale: that many times as many, shorter row ranges (2 under the data-parallel step: see include/clvae.h)."""
    L = _lib.lib()
    buf, job = _scratch(L.clv_lstm_wgrad_workspace_bytes(K, N, nx, nh, nz, int(split_scale)), ws, defer)
    check(L.clv_lstm_wgrad(K, N, _ptr(X), ldx, nx, _frames_mode(X, x_exact_bf16), _ptr(H), ldh, nh, 1, T,
                              _ptr(Z), ldz, nz, _ptr(dz), N, _ptr(dKx), N, _ptr(dU), N, _ptr(dKz), N, float(beta),
                              int(split_scale), _ptr(buf), buf.numel(), job, _stream()), "clv_lstm_wgrad")


def _wgrad_problem(K, N, X, ldx, nx, x_exact_bf16, H, ldh, nh, T, Z, ldz, nz, dz, dKx, dU, dKz, beta=0.0):
    w = _lib.WgradProblem()
    w.K, w.N = K, N
    w.X, w.ldx, w.nx, w.x_exact_bf16 = _ptr(X), ldx, nx, _frames_mode(X, x_exact_bf16)
    w.H, w.ldh, w.nh, w.h_shift, w.h_zero_period = _ptr(H), ldh, nh, 1, T
    w.Z, w.ldz, w.nz = _ptr(Z), ldz, nz
    w.dz, w.lddz = _ptr(dz), N
    w.dKx, w.ld_kx, w.dU, w.ld_u, w.dKz, w.ld_kz = _ptr(dKx), N, _ptr(dU), N, _ptr(dKz), N
    w.beta = float(beta)
    return w


def lstm_wgrad_pair_supported(p, q):
    """p, q: the argument tuples of lstm_wgrad up to dKz (K, N, X, ldx, nx, x_exact_bf16, H, ldh, nh, T, Z, ldz, nz, dz, dKx,
    dU, dKz): can both products run as ONE launch (clv_lstm_wgrad_pair)?"""
    a, b = _wgrad_problem(*p), _wgrad_problem(*q)
    return bool(_lib.lib().clv_lstm_wgrad_pair_supported(C.byref(a), C.byref(b)))


def lstm_wgrad_pair(p, q, ws, defer=None, split_scale=1):
    """Both LSTMs' kernel gradients of a step in one launch (csrc/wgrad_bf16.hip: row ranges twice as long, half as many
    slabs); p, q as in lstm_wgrad_pair_supported.  ws: a pair of Workspaces when the reductions are not deferred."""
    L = _lib.lib()
    probs, jobs = [], []
    for i, t in enumerate((p, q)):
        w = _wgrad_problem(*t)
        need = L.clv_lstm_wgrad_pair_workspace_bytes(w.K, w.N, w.nx, w.nh, w.nz, int(split_scale))
        buf, job = _scratch(need, ws[i] if defer is None else None, defer)
        jobs.append(job)
        w.ws, w.ws_bytes = _ptr(buf), buf.numel()
        probs.append(w)
    check(L.clv_lstm_wgrad_pair(C.byref(probs[0]), C.byref(probs[1]), int(split_scale), jobs[0], jobs[1], _stream()),
          "clv_lstm_wgrad_pair")


def gemm_bce(A, B, bias, Y, scale, logits, dlogits, rownll, M, N, K, lda=None, ldb=None, ldy=None, ldc=None):
    """Output head + Bernoulli NLL in one launch: logits = A.B + bias, rownll, dlogits = scale*(sigmoid - Y)."""
    check(_lib.lib().clv_gemm_bce_f32(M, N, K, _ptr(A), lda if lda is not None else K, _ptr(B),
                                      ldb if ldb is not None else N, _ptr(bias), _ptr(Y), ldy if ldy is not None else N,
                                      float(scale), _ptr(logits), _ptr(dlogits), ldc if ldc is not None else N,
                                      _ptr(rownll), _stream()), "clv_gemm_bce_f32")


def out_head_train_supported(H, D):
    return bool(_lib.lib().clv_out_head_train_supported(H, D))


def out_head_train(R, H, D, hs, Wo, bo, Y, scale, rownll, dhs, dWo, dbo, ws, logits=None, dlogits=None, ldy=None,
                   defer=None):
    """Output head forward + Bernoulli NLL + dhs + dWo/dbo in one launch (see clv_out_head_train).  Y: the target frames,
    float32 or the bytes themselves (uint8).
    defer: a ReduceQueue that takes the pending reduction of the weight-gradient slabs."""
    L = _lib.lib()
    buf, job = _scratch(L.clv_out_head_train_workspace_bytes(R), ws, defer)
    check(L.clv_out_head_train(R, H, D, _ptr(hs), _ptr(Wo), _ptr(bo), _ptr(Y), _is_u8(Y), ldy if ldy is not None else D,
                               float(scale), _ptr(logits), _ptr(rownll), _ptr(dlogits), _ptr(dhs), _ptr(dWo), _ptr(dbo),
                               _ptr(buf), buf.numel(), job, _stream()), "clv_out_head_train")


def latent_head_supported(H, L):
    return bool(_lib.lib().clv_latent_head_supported(H, L))


def latent_head_fwd(R, H, L, hs, Wz, bz, eps, zargs, Z, ldz, rowkl=None, noise=None):
    """zargs = hs.Wz + bz, the reparametrised sample into Z (row stride ldz) and the rows' KL in one launch.
    noise (noise_draw(...)): eps is drawn inside the kernel and written to `eps`, else read from it."""
    check(_lib.lib().clv_latent_head_fwd(R, H, L, _ptr(hs), _ptr(Wz), _ptr(bz), _ptr(eps), _ptr(zargs), _ptr(Z), ldz,
                                         _ptr(rowkl), _noise_ref(noise), _stream()), "clv_latent_head_fwd")


def latent_head_bwd(R, H, L, hs, Wz, zargs, eps, dZ, lddz, kl_scale, dhs, dWz, dbz, ws, dzargs=None, defer=None):
    """The latent head's backward in one launch: dzargs (kept on chip unless a buffer is given), dhs = dzargs.Wz^T and the
    layer's kernel / bias gradient.  defer: a ReduceQueue that takes the pending reduction of the weight-gradient slabs."""
    Lb = _lib.lib()
    buf, job = _scratch(Lb.clv_latent_head_bwd_workspace_bytes(R, L), ws, defer)
    check(Lb.clv_latent_head_bwd(R, H, L, _ptr(hs), _ptr(Wz), _ptr(zargs), _ptr(eps), _ptr(dZ), lddz, float(kl_scale),
                                 _ptr(dzargs), _ptr(dhs), _ptr(dWz), _ptr(dbz), _ptr(buf), buf.numel(), job, _stream()),
          "clv_latent_head_bwd")


def gemm_grouped_tn_small2(probs0, B0, probs1, B1, N, K, ldb=None):
    """Two few-row grouped products (different B operands) in one launch; see clv_gemm_grouped_tn_small2."""
    a0, a1 = _prob_array(probs0, N), _prob_array(probs1, N)
    check(_lib.lib().clv_gemm_grouped_tn_small2(a0, len(probs0), _ptr(B0), a1, len(probs1), _ptr(B1), N, K,
                                                ldb if ldb is not None else N, _stream()), "clv_gemm_grouped_tn_small2")


def loss_sums(terms, out):
    """terms: five (tensor, n, stride); out[k] = mean of term k."""
    a = []
    for t, n, st in terms:
        a += [_ptr(t), n, st]
    check(_lib.lib().clv_loss_sums(*a, _ptr(out), _stream()), "clv_loss_sums")


def colsum(X, M, N, out, ws, ldx=None, beta=0.0):
    L = _lib.lib()
    buf = ws.ensure(L.clv_colsum_workspace_bytes(M, N))
    check(L.clv_colsum_f32(M, N, _ptr(X), ldx if ldx is not None else N, float(beta), _ptr(out), _ptr(buf),
                           buf.numel(), _stream()), "clv_colsum_f32")


def lstm_seq_fwd(B, T, xproj, rowbias, U, hs, cs, gates, h0=None, c0=None, hT=None, cT=None, gate_act=0, H=88):
    check(_lib.lib().clv_lstm_seq_fwd(B, T, H, gate_act, _ptr(xproj), _ptr(rowbias), _ptr(U), _ptr(h0), _ptr(c0),
                                      _ptr(hs), _ptr(cs), _ptr(gates), _ptr(hT), _ptr(cT), _stream()),
          "clv_lstm_seq_fwd")


def lstm_seq_bwd_z(B, T, U, dhs, cs, gates_inout, dzsum, Kz, nz, dZ, lddz, c0=None, gate_act=0, H=88):
    """clv_lstm_seq_bwd + dZ = dz . Kz^T in the same launch."""
    check(_lib.lib().clv_lstm_seq_bwd_z(B, T, H, gate_act, _ptr(U), _ptr(dhs), _ptr(cs), _ptr(c0), _ptr(gates_inout),
                                        _ptr(dzsum), _ptr(Kz), nz, _ptr(dZ), lddz, _stream()), "clv_lstm_seq_bwd_z")


def lstm_seq_bwd(B, T, U, dhs, cs, gates_inout, dzsum, c0=None, gate_act=0, H=88):
    check(_lib.lib().clv_lstm_seq_bwd(B, T, H, gate_act, _ptr(U), _ptr(dhs), _ptr(cs), _ptr(c0), _ptr(gates_inout),
                                      _ptr(dzsum), _stream()), "clv_lstm_seq_bwd")


def lstm_mx_supported(B, nx, nz, H=88):
    """the large-batch LSTM kernels on the bf16 matrix cores (csrc/lstm_mx.hip) take this shape"""
    return bool(_lib.lib().clv_lstm_mx_supported(B, H, nx, nz))


def lstm_mx_fwd(B, T, X, ldx, nx, Kx, Z, ldz, nz, Kz, rowbias, U, hs, coef, aux, gate_act=0, H=88):
    """LSTM training forward with the input products inside the kernel: frames X (sparse rows of Kx; float32 or the bytes
    themselves, ldx in elements) and latents Z."""
    check(_lib.lib().clv_lstm_mx_fwd(B, T, H, gate_act, _ptr(X), _is_u8(X) if X is not None else 0, ldx, nx, _ptr(Kx), _ptr(Z), ldz, nz, _ptr(Kz),
                                     _ptr(rowbias), _ptr(U), _ptr(hs), _ptr(coef), _ptr(aux), _stream()), "clv_lstm_mx_fwd")


def lstm_mx_bwd(B, T, U, dhs, aux, coef_inout, dzsum, Kz=None, nz=0, dZ=None, lddz=0, H=88):
    """BPTT of lstm_mx_fwd; coef_inout becomes dz; nz > 0: dZ = dz . Kz^T from the same launch."""
    check(_lib.lib().clv_lstm_mx_bwd(B, T, H, _ptr(U), _ptr(dhs), _ptr(aux), _ptr(coef_inout), _ptr(dzsum), _ptr(Kz), nz,
                                     _ptr(dZ), lddz, _stream()), "clv_lstm_mx_bwd")


def sparse_proj_supported(nx, N):
    return bool(_lib.lib().clv_sparse_proj_supported(nx, N))


def sparse_proj2(R, N, a, b, ldo=None):
    """Two projections over the same R frames in one launch; a, b = (nx, X, ldx, K, out); X float32, or both the bytes themselves."""
    if _is_u8(a[1]) != _is_u8(b[1]):
        raise TypeError("both projections read float frames or both read bytes")
    check(_lib.lib().clv_sparse_proj2(R, N, ldo if ldo is not None else N, _is_u8(a[1]), a[0], _ptr(a[1]), a[2], _ptr(a[3]), _ptr(a[4]),
                                      b[0], _ptr(b[1]), b[2], _ptr(b[3]), _ptr(b[4]), _stream()), "clv_sparse_proj2")


def sparse_proj(R, nx, N, X, ldx, K, out, ldo=None):
    """out[r,:N] = sum_k X[r,k] K[k,:] visiting only the nonzero inputs of a frame (K resident in LDS)."""
    check(_lib.lib().clv_sparse_proj(R, nx, N, _ptr(X), _is_u8(X), ldx, _ptr(K), _ptr(out), ldo if ldo is not None else N,
                                     _stream()), "clv_sparse_proj")


def sparse_dense_supported(N):
    return bool(_lib.lib().clv_sparse_dense_supported(N))


def sparse_dense(R, nx, N, X, ldx, K, bias, act, out, ldo=None):
    """out[r,:N] = act(sum_j X[r,j] K[j,:] + bias) over the nonzero inputs of each row (K read from HBM/L2)."""
    check(_lib.lib().clv_sparse_dense(R, nx, N, _ptr(X), ldx, _ptr(K), _ptr(bias), act, _ptr(out),
                                      ldo if ldo is not None else N, _stream()), "clv_sparse_dense")


def sparse_outer(Bn, nx, N, X, ldx, G, ldg, out, ldo=None, colsum=None, gdot=None):
    """out[j,:N] = sum_b X[b,j] G[b,:] (kernel gradient of a Dense layer with sparse inputs); colsum[N] = sum_b G[b,:].
    gdot = (Hact, ldh, hbias, out[N]): also sum_b (Hact - hbias)[b,c] G[b,c] = sum_j K[j,c] dK[j,c] (the `known` sums of clv_adam_wn_step)."""
    h, ldh, hb, go = gdot if gdot is not None else (None, 0, None, None)
    check(_lib.lib().clv_sparse_outer(Bn, nx, N, _ptr(X), ldx, _ptr(G), ldg, _ptr(out), ldo if ldo is not None else N,
                                         _ptr(colsum), _ptr(h), int(ldh), _ptr(hb), _ptr(go), _stream()), "clv_sparse_outer")


def dense_outer_bf16_supported(Bn, nx, N, ldx, ldg):
    return bool(_lib.lib().clv_dense_outer_bf16_supported(Bn, nx, N, ldx, ldg))


def dense_outer_bf16(Bn, nx, N, X, ldx, G, ldg, out, ldo=None, colsum=None, gdot=None):
    """sparse_outer's product for inputs that are exactly bf16 numbers (frames kept as bytes), dense on the bf16 matrix cores
    (csrc/outer_bf16.hip); same arguments.  X: float32, or the bytes themselves (uint8; ldx in elements either way)."""
    h, ldh, hb, go = gdot if gdot is not None else (None, 0, None, None)
    check(_lib.lib().clv_dense_outer_bf16(Bn, nx, N, _ptr(X), _is_u8(X), ldx, _ptr(G), ldg, _ptr(out), ldo if ldo is not None else N,
                                          _ptr(colsum), _ptr(h), int(ldh), _ptr(hb), _ptr(go), _stream()), "clv_dense_outer_bf16")


def _ptrs(*tensors):
    return [_ptr(t) for t in tensors]


def _sample(name, *args):
    """one entry point of the persistent sampling kernels: name(*args, stream), checked"""
    check(getattr(_lib.lib(), name)(*args, _stream()), name)


def _temper(temper):
    """the flag and the two factors of a sampling entry point: None is the untempered call (0, 1.0, 1.0)"""
    inv_T, Tz = (1.0, 1.0) if temper is None else temper
    return [int(temper is not None), float(inv_T), float(Tz)]


def vrnn_generate_supported(D, H, L, Cn):
    return bool(_lib.lib().clv_vrnn_generate_supported(D, H, L, Cn))


def vrnn_generate(N, S, nsteps, D, H, L, Cn, gate_act, z_prior, seed, x_seed, w, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz,
                  Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo, Xs, xhat=None, clamp=None, temper=None, t0=0, state_in=None,
                  state_out=None):
    """cl_vrnn frame loop for N sequences in one persistent launch (clv_vrnn_generate, csrc/generate.hip); clamp: uint8
    [N,nsteps,D] constraint roll or None; temper: None or (inv_temperature, z_temperature), the tempered model's two factors.
    From and to a state once t0, state_in or state_out is given: t0 the Philox step of the call's frame 0,
    state_in / state_out [N,5,88] (h_enc, c_enc, h_dec, c_dec, x; either may be None, they may be one tensor); then x_seed
    may be None with S = 0 and Xs None with nsteps = 0."""
    _sample("clv_vrnn_generate", N, S, nsteps, D, H, L, Cn, gate_act, int(bool(z_prior)), int(seed),
            *_ptrs(x_seed, w, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo, clamp),
            *_temper(temper), int(t0), *_ptrs(state_in, state_out, Xs, xhat))


def vae_generate_supported(D, H, L, Cn):
    return bool(_lib.lib().clv_vae_generate_supported(D, H, L, Cn))


def vae_generate(N, nsteps, D, H, L, Cn, use_x_prev, z_prior, seed, x_seed, w, Kh, bh, Kz, bz, Kd, bd, Ko, bo, Xs, xhat=None,
                 clamp=None, temper=None, t0=0, state_in=None, state_out=None):
    """cl_vae frame loop for N sequences in one persistent launch (clv_vae_generate, csrc/vae_generate.hip); clamp, temper,
    t0 as vrnn_generate's.  From and to a state: state_in [N,2,88] (x_in, hist) stands for the seed frame, so x_seed is
    None; state_out may be None or state_in."""
    _sample("clv_vae_generate", N, nsteps, D, H, L, Cn, int(bool(use_x_prev)), int(bool(z_prior)), int(seed),
            *_ptrs(x_seed, w, Kh, bh, Kz, bz, Kd, bd, Ko, bo, clamp), *_temper(temper), int(t0),
            *_ptrs(state_in, state_out, Xs, xhat))


def vrnn_vary(N, T, D, H, L, Cn, gate_act, hist_source, seed, sources, x0, w_enc, w_dec, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz,
              Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo, Xs, xhat=None, clamp=None, temper=None, zout=None):
    """cl_vrnn re-decoding of sources [N,T,D] in one persistent launch (clv_vrnn_vary); x0, clamp, xhat may be
    None; temper: None or (inv_temperature, z_temperature); zout [3,N,T,L] = (z_mean, z_log_var, z) also stores the latents
    (DESIGN.md 15)."""
    _sample("clv_vrnn_vary", N, T, D, H, L, Cn, gate_act, int(bool(hist_source)), int(seed),
            *_ptrs(sources, x0, w_enc, w_dec, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo, clamp),
            *_temper(temper)[1:], *_ptrs(Xs, xhat, zout))


def vae_vary(N, T, D, H, L, Cn, use_x_prev, hist_source, seed, sources, x0, w_enc, w_dec, Kh, bh, Kz, bz, Kd, bd, Ko, bo, Xs,
             xhat=None, clamp=None, temper=None, zout=None):
    """cl_vae re-decoding of sources [N,T,D] in one persistent launch (clv_vae_vary); arguments as vrnn_vary"""
    _sample("clv_vae_vary", N, T, D, H, L, Cn, int(bool(use_x_prev)), int(bool(hist_source)), int(seed),
            *_ptrs(sources, x0, w_enc, w_dec, Kh, bh, Kz, bz, Kd, bd, Ko, bo, clamp), *_temper(temper)[1:], *_ptrs(Xs, xhat, zout))


def vrnn_decode(N, T, D, H, L, Cn, gate_act, seed, z_in, x0, history, w_dec, noise_rows, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo,
                bo, Xs, xhat=None, clamp=None, inv_T=1.0):
    """cl_vrnn decoding of the latent path z_in [N,T,L] in one persistent launch (clv_vrnn_decode); x0, history
    [N,T,D], noise_rows [N] int32 (entries >= 0: validated by the caller), clamp, xhat may be None"""
    _sample("clv_vrnn_decode", N, T, D, H, L, Cn, gate_act, int(seed),
            *_ptrs(z_in, x0, history, w_dec, noise_rows, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo, clamp), float(inv_T), *_ptrs(Xs, xhat))


def vae_decode(N, T, D, H, L, Cn, use_x_prev, seed, z_in, x0, history, w_dec, noise_rows, Kd, bd, Ko, bo, Xs, xhat=None,
               clamp=None, inv_T=1.0):
    """cl_vae decoding of the latent path z_in [N,T,L] in one persistent launch (clv_vae_decode); arguments as vrnn_decode"""
    _sample("clv_vae_decode", N, T, D, H, L, Cn, int(bool(use_x_prev)), int(seed),
            *_ptrs(z_in, x0, history, w_dec, noise_rows, Kd, bd, Ko, bo, clamp), float(inv_T), *_ptrs(Xs, xhat))


def lerp_rows(R, n, a, ia, b, ib, alpha, out):
    """out [R, n] = (1 - alpha[r]) a[ia[r]] + alpha[r] b[ib[r]] as two fmas, exact at both ends (clv_lerp_rows); ia, ib int32"""
    check(_lib.lib().clv_lerp_rows(int(R), int(n), _ptr(a), _ptr(ia), _ptr(b), _ptr(ib), _ptr(alpha), _ptr(out), _stream()),
          "clv_lerp_rows")


def take_frame(R, T, D, src, step_dev, out):
    """out [R, D] = src[:, *step_dev] of src [R, T, D]: a captured frame chain's read of its source (clv_take_frame)"""
    check(_lib.lib().clv_take_frame(int(R) * int(D), int(T), int(D), _ptr(src), _ptr(step_dev), _ptr(out), _stream()),
          "clv_take_frame")


def lstm_pair_supported(L, H=88):
    return bool(_lib.lib().clv_lstm_pair_supported(H, L))


def lstm_pair_pack_floats():
    return int(_lib.lib().clv_lstm_pair_pack_floats())


def lstm_pair_pack(L, U_enc, U_dec, Kz, Wz, pack, H=88):
    """Recurrent kernels, Kz and Wz in the lane order of the pair kernels (once per weight update)."""
    check(_lib.lib().clv_lstm_pair_pack(H, L, _ptr(U_enc), _ptr(U_dec), _ptr(Kz), _ptr(Wz), _ptr(pack), _stream()),
          "clv_lstm_pair_pack")


def lstm_pair_fwd(B, T, L, gates_enc, rb_enc, gates_dec, dec_has_xproj, rb_dec, pack, bz, eps,
                  hs_enc, aux_enc, hs_dec, aux_dec, zargs, Z, ldz, klterm, gate_act=0, H=88, noise=None, notes=None):
    """aux_* [B*T, 2H]: (kcarry, kc) of the backward pass; noise: a noise_draw(): eps is drawn in the kernel;
    notes = (notes_enc, Kx_enc, notes_dec, Kx_dec): the input projections are gathered in the kernel from note lists
    (gather_rows_multi(notes=...)) and the kernels' frame rows; gates_* are then outputs only."""
    ne, ke, nd, kd = notes if notes is not None else (None, None, None, None)
    check(_lib.lib().clv_lstm_pair_fwd(B, T, H, L, gate_act, _ptr(gates_enc), _ptr(rb_enc), _ptr(gates_dec),
                                       int(bool(dec_has_xproj)), _ptr(rb_dec), _ptr(pack), _ptr(bz),
                                       _ptr(eps), _ptr(hs_enc), _ptr(aux_enc), _ptr(hs_dec), _ptr(aux_dec), _ptr(zargs),
                                       _ptr(Z), ldz, _ptr(klterm), _ptr(ne), _ptr(ke), _ptr(nd), _ptr(kd), _noise_ref(noise),
                                       _stream()), "clv_lstm_pair_fwd")


def lstm_pair_bwd(B, T, L, kl_scale, pack, Wz, dhs_dec, aux_dec, aux_enc, gates_dec, gates_enc, dzsum_dec,
                  dzsum_enc, zargs, eps, dzargs, gate_act=0, H=88, head_grad=None, ws=None, defer=None, label=None):
    """head_grad = (hs_enc, dWz, dbz): the latent head's kernel / bias gradient is accumulated inside the kernel (per-row
    slabs, summed by the pending reduction of `defer`, or at once) instead of by a GEMM over hs_enc.
    label = dict(D, C, Kenc_w, Kdec_w, wargs, eps, onehot, W, hW, Ka, prior, class_weight, w_kl_weight, inv_b, dwargs, dhW,
    layer_grad=(dKa, dba) | None): the label path's backward (vrnn_label_bwd) as the kernel's epilogue."""
    Lb = _lib.lib()
    hs, dWz, dbz = head_grad if head_grad is not None else (None, None, None)
    lg = label.get('layer_grad') if label is not None else None
    need_h = Lb.clv_lstm_pair_bwd_workspace_bytes(B, H, L) if head_grad is not None else None
    need_l = Lb.clv_vrnn_label_bwd_workspace_bytes(B, label['D'], label['C']) if lg is not None else None
    (hptr, job), (lptr, ljob) = _scratch_regions((need_h, need_l), ws, defer)      # the head's slot first, then the label's
    rider = None
    if label is not None:
        rider = _lib.LabelBwdRider(label['D'], label['C'], _ptr(label['Kenc_w']), _ptr(label['Kdec_w']), _ptr(label['wargs']),
                                   _ptr(label['eps']), _ptr(label['onehot']), _ptr(label['W']), _ptr(label['hW']),
                                   _ptr(label['Ka']), float(label['prior']), float(label['class_weight']),
                                   float(label['w_kl_weight']), float(label['inv_b']), _ptr(label['dwargs']),
                                   _ptr(label['dhW']), _ptr(lg[0]) if lg else None, _ptr(lg[1]) if lg else None,
                                   lptr, need_l or 0, ljob)
    check(Lb.clv_lstm_pair_bwd(B, T, H, L, gate_act, float(kl_scale), _ptr(pack), _ptr(Wz),
                                  _ptr(dhs_dec), _ptr(aux_dec), _ptr(aux_enc), _ptr(gates_dec), _ptr(gates_enc),
                                  _ptr(dzsum_dec), _ptr(dzsum_enc), _ptr(zargs), _ptr(eps), _ptr(dzargs),
                                  _ptr(hs), _ptr(dWz), _ptr(dbz), hptr, need_h or 0, job,
                                  C.byref(rider) if rider is not None else None, _stream()),
          "clv_lstm_pair_bwd")


def label_fwd(B, Cn, mean, logvar, ld_in, eps, onehot, prior, w, rowloss):
    check(_lib.lib().clv_label_fwd(B, Cn, _ptr(mean), _ptr(logvar), ld_in, _ptr(eps), _ptr(onehot), float(prior),
                                   _ptr(w), _ptr(rowloss), _stream()), "clv_label_fwd")


def label_bwd(B, Cn, mean, logvar, ld_in, eps, onehot, w, dw, prior, class_weight, w_kl_weight, inv_b,
              dmean, dlogvar, ld_out):
    check(_lib.lib().clv_label_bwd(B, Cn, _ptr(mean), _ptr(logvar), ld_in, _ptr(eps), _ptr(onehot), _ptr(w), _ptr(dw),
                                   float(prior), float(class_weight), float(w_kl_weight), float(inv_b),
                                   _ptr(dmean), _ptr(dlogvar), ld_out, _stream()), "clv_label_bwd")


def vrnn_label_fwd(B, D, Cn, G4, hW, Ka, ba, eps, onehot, prior, Kenc_w, benc, Kdec_w, bdec, wargs, W, rowloss, rb_enc,
                   rb_dec):
    check(_lib.lib().clv_vrnn_label_fwd(B, D, Cn, G4, _ptr(hW), _ptr(Ka), _ptr(ba), _ptr(eps), _ptr(onehot),
                                        float(prior), _ptr(Kenc_w), _ptr(benc), _ptr(Kdec_w), _ptr(bdec), _ptr(wargs),
                                        _ptr(W), _ptr(rowloss), _ptr(rb_enc), _ptr(rb_dec), _stream()),
          "clv_vrnn_label_fwd")


def noise_draw(seed, stream, first, step=0, step_dev=None):
    """clv_noise_draw: the kernel that gets it draws eps itself (the clv_philox_normal values at indices first + e) and
    writes them to its eps buffer.  The struct is returned by value: keep it alive across the call (ctypes copies the
    fields when the launch is made / captured)."""
    return _lib.NoiseDraw(int(seed), int(first), int(stream), int(step), _ptr(step_dev))


def _is_u8(t):
    """1 for a uint8 tensor (frames kept as bytes), 0 for float32: the x_u8 flag of the entry points that take either"""
    if t.dtype == torch.uint8:
        return 1
    if t.dtype != torch.float32:
        raise TypeError("frames must be float32 or uint8, got %s" % t.dtype)
    return 0


def _frames_mode(X, exact):
    """CLV_FRAMES_* of include/clvae.h: 2 = X holds the frames as bytes, 1 = float values that are exactly bf16 numbers, 0 = any"""
    return 2 if _is_u8(X) else int(bool(exact))


def _noise_ref(noise):
    return C.byref(noise) if noise is not None else None


def label_stage(cur, hist, idx, row0, cursor, X, Xh, hist_chunk, hist_ld, w_src, w_out, bytes_out=None):
    """clv_label_stage for vrnn_label_fwd_x(stage=...): cur / hist = (uint8 store, stride, offset, table or None) of the
    current / history frames (hist None: no history frames), cursor = (step_dev, step0, period, stride, offset) or None.
    bytes_out = (X8, Xh8): the rows are copied as bytes into these uint8 [B, nx] buffers instead of widened into X / Xh."""
    g = _lib.LabelStage()
    g.cur, g.cur_stride, g.cur_offset, g.cur_table = _ptr(cur[0]), int(cur[1]), int(cur[2]), _ptr(cur[3])
    if hist is not None:
        g.hist, g.hist_stride, g.hist_offset, g.hist_table = _ptr(hist[0]), int(hist[1]), int(hist[2]), _ptr(hist[3])
    g.idx, g.row0 = _ptr(idx), int(row0)
    if cursor is not None:
        g.cursor = _lib.BatchCursor(_ptr(cursor[0]), int(cursor[1]), int(cursor[2]), int(cursor[3]), int(cursor[4]))
    g.X, g.Xh, g.hist_chunk, g.hist_ld = _ptr(X), _ptr(Xh), int(hist_chunk), int(hist_ld)
    g.w_src, g.w_out = _ptr(w_src), _ptr(w_out)
    if bytes_out is not None:
        g.X8, g.Xh8 = _ptr(bytes_out[0]), _ptr(bytes_out[1])
    return g


def vrnn_label_fwd_x_proj_supported(B, D, nx, T, N):
    return bool(_lib.lib().clv_vrnn_label_fwd_x_proj_supported(B, D, nx, T, N))


def vrnn_label_fwd_x(B, D, Cn, G4, X, ldx, nx, Kh, bh, hW_out, Ka, ba, eps, onehot, prior, Kenc_w, benc, Kdec_w, bdec, wargs,
                     W, rowloss, rb_enc, rb_dec, noise=None, pack=None, parts=None, stage=None, proj=None):
    """hW = relu(X . Kh + bh) over the nonzero inputs of each row, then vrnn_label_fwd, one workgroup per row.
    noise: a noise_draw(): eps is drawn in the kernel (and written to `eps`) instead of read.
    pack = (L, U_enc, U_dec, Kz, Wz, out): the launch also writes the pair LSTM kernels' weight pack (lstm_pair_pack).
    parts = (buffer, splits): X . Kh was formed by dense_window_fwd_bf16 as split-K partial sums; X / Kh are not read.
    proj = (T, N, K_cur, out_cur, K_hist or None, out_hist or None): the launch also forms the LSTMs' frame projections of the
    staged rows (sparse_proj2's outputs bit for bit; needs a stage with bytes_out)."""
    pj = None
    if proj is not None:
        if stage is None or parts is not None:
            raise ValueError("proj rides on a stage (the byte stores it names), not on parts")
        T_, N_, kc, oc, kh, oh = proj
        pj = _lib.FrameProj(int(T_), int(N_), int(N_), _ptr(kc), _ptr(oc), _ptr(kh), _ptr(oh))
    ps = None
    if pack is not None:
        L_, ue, ud, kz, wz, out = pack
        ps = _lib.PairPackSrc(88, int(L_), _ptr(ue), _ptr(ud), _ptr(kz), _ptr(wz), _ptr(out))
    tail = (_ptr(bh), _ptr(hW_out), _ptr(Ka), _ptr(ba), _ptr(eps), _ptr(onehot), float(prior), _ptr(Kenc_w), _ptr(benc),
            _ptr(Kdec_w), _ptr(bdec), _ptr(wargs), _ptr(W), _ptr(rowloss), _ptr(rb_enc), _ptr(rb_dec), _noise_ref(noise),
            C.byref(ps) if ps is not None else None, _stream())
    if parts is not None and stage is None:
        check(_lib.lib().clv_vrnn_label_fwd_parts(B, D, Cn, G4, _ptr(parts[0]), int(parts[1]), *tail), "clv_vrnn_label_fwd_parts")
    else:      # stage = a label_stage(): the launch assembles the mini-batch rows itself (X, history frames, labels)
        check(_lib.lib().clv_vrnn_label_fwd_x(B, D, Cn, G4, _ptr(X), ldx, nx, _ptr(Kh), C.byref(stage) if stage is not None else None,
                                              *tail[:-1], C.byref(pj) if pj is not None else None, tail[-1]), "clv_vrnn_label_fwd_x")


def dense_window_fwd_bf16_supported(Bn, nx, N, ldx, ldk):
    return bool(_lib.lib().clv_dense_window_fwd_bf16_supported(Bn, nx, N, ldx, ldk))


def dense_window_fwd_bf16(Bn, nx, N, X, ldx, K, ldk, ws):
    """X . K for byte-valued X as split-K partial sums on the bf16 matrix cores (csrc/outer_bf16.hip); returns (buffer, splits)
    for vrnn_label_fwd_x(parts=...).  ws: a Workspace that keeps the buffer."""
    L = _lib.lib()
    buf = ws.ensure(L.clv_dense_window_fwd_bf16_workspace_bytes(Bn, nx, N))
    check(L.clv_dense_window_fwd_bf16(Bn, nx, N, _ptr(X), _is_u8(X), ldx, _ptr(K), ldk, _ptr(buf), buf.numel(), _stream()),
          "clv_dense_window_fwd_bf16")
    return buf, L.clv_dense_window_fwd_bf16_splits(Bn, nx)


def vrnn_label_bwd(B, D, Cn, G4, dzsum_enc, dzsum_dec, Kenc_w, Kdec_w, wargs, eps, onehot, W, hW, Ka, prior,
                   class_weight, w_kl_weight, inv_b, dwargs, dhW, layer_grad=None, ws=None, defer=None):
    """layer_grad = (dKa, dba): the Wargs layer's kernel / bias gradient as per-row slabs summed by `defer`'s pending
    reductions (or at once) instead of a GEMM over K = batch."""
    Lb = _lib.lib()
    dKa, dba, buf, nbytes, job = None, None, None, 0, None
    if layer_grad is not None:
        dKa, dba = layer_grad
        buf, job = _scratch(Lb.clv_vrnn_label_bwd_workspace_bytes(B, D, Cn), ws, defer)
        nbytes = buf.numel()
    check(Lb.clv_vrnn_label_bwd(B, D, Cn, G4, _ptr(dzsum_enc), _ptr(dzsum_dec), _ptr(Kenc_w), _ptr(Kdec_w),
                                   _ptr(wargs), _ptr(eps), _ptr(onehot), _ptr(W), _ptr(hW), _ptr(Ka),
                                   float(prior), float(class_weight), float(w_kl_weight), float(inv_b),
                                   _ptr(dwargs), _ptr(dhW), _ptr(dKa), _ptr(dba), _ptr(buf), nbytes, job, _stream()),
          "clv_vrnn_label_bwd")


def gauss_fwd(R, Ld, zargs, eps, z, ldz, rowkl):
    check(_lib.lib().clv_gauss_fwd(R, Ld, _ptr(zargs), _ptr(eps), _ptr(z), ldz, _ptr(rowkl), _stream()),
          "clv_gauss_fwd")


def gauss_bwd(R, Ld, zargs, eps, dz, lddz, kl_scale, dzargs):
    check(_lib.lib().clv_gauss_bwd(R, Ld, _ptr(zargs), _ptr(eps), _ptr(dz), lddz, float(kl_scale), _ptr(dzargs),
                                   _stream()), "clv_gauss_bwd")


def bernoulli_nll(R, D, logits, y, ldy, scale, rownll, dlogits):
    check(_lib.lib().clv_bernoulli_nll(R, D, _ptr(logits), _ptr(y), ldy, float(scale), _ptr(rownll), _ptr(dlogits),
                                       _stream()), "clv_bernoulli_nll")


def sum_strided(n, x, stride, scale, out):
    check(_lib.lib().clv_sum_strided(n, _ptr(x), stride, float(scale), _ptr(out), _stream()), "clv_sum_strided")


def axpy(n, alpha, x, y):
    check(_lib.lib().clv_axpy(n, float(alpha), _ptr(x), _ptr(y), _stream()), "clv_axpy")


def gather_rows(rows, row_elems, src, idx, out, chunk=0, out_ld=0):
    check(_lib.lib().clv_gather_rows(rows, row_elems, _ptr(src), _ptr(idx), _ptr(out), chunk, out_ld, _stream()),
          "clv_gather_rows")


NOTE_ROW, NOTE_NONE = 96, 88       # CLV_NOTE_ROW / CLV_NOTE_NONE (include/clvae.h)


def _gather_args(segs, notes, cursor):
    """the segment arrays, note outputs and batch cursor of gather_rows_multi / gather_transposed as ctypes arguments"""
    n = len(segs)
    P, I, U = C.c_void_p * n, C.c_int64 * n, C.c_int32 * n
    src = P(*[s_[0].data_ptr() for s_ in segs])
    if any(s_[1].dtype == torch.uint8 and s_[0].dtype != torch.uint8 for s_ in segs):
        raise TypeError("a uint8 output takes a uint8 source")
    # 2: bytes in, bytes out (a batch that stays uint8, out_ld in bytes); 1: bytes widened to float; 0: float
    u8 = U(*[(2 if s_[1].dtype == torch.uint8 else 1) if s_[0].dtype == torch.uint8 else 0 for s_ in segs])
    out = P(*[s_[1].data_ptr() for s_ in segs])
    re = I(*[int(s_[2]) for s_ in segs])
    ch = I(*[int(s_[3]) for s_ in segs])
    ld = I(*[int(s_[4]) for s_ in segs])
    ext = [tuple(s_[5:8]) + (0, 0, None)[len(s_[5:8]):] for s_ in segs]
    st = I(*[int(e[0]) for e in ext])
    of = I(*[int(e[1]) for e in ext])
    tb = P(*[(e[2].data_ptr() if e[2] is not None else None) for e in ext])
    nt = P(*[(t.data_ptr() if t is not None else None) for t in (notes or [None] * n)])
    cur = None      # (step_dev int32 tensor, step0, period, stride, offset): the batch is chosen on the device
    if cursor is not None:
        cur = C.byref(_lib.BatchCursor(cursor[0].data_ptr(), int(cursor[1]), int(cursor[2]), int(cursor[3]), int(cursor[4])))
    return n, src, u8, out, re, ch, ld, st, of, tb, nt, cur


def gather_rows_multi(rows, idx, segs, row0=0, notes=None, cursor=None):
    """segs: up to 4 (src, out, row_elems, chunk, out_ld[, stride, offset, table]); one launch; idx None = rows
    row0..row0+rows-1.  A uint8 src (binary frames kept as bytes) is converted to float on the way -- or copied as bytes when
    `out` is a uint8 tensor too.  With (stride,
    offset, table) source row r starts at element table[idx[r]] * stride + offset: windows of a frame store.
    notes: per segment None or a uint8 tensor [rows * pieces, NOTE_ROW] that receives the frames' note lists (uint8
    sources of binary frames only): what lstm_pair_fwd gathers the input projections from.
    cursor = (step_dev, step0, period, stride, offset): batch j = (step - step0) mod period, rows j * stride + offset ..
    of the row list, chosen by the launch itself from the device step counter (a node of the step's graph)."""
    n, src, u8, out, re, ch, ld, st, of, tb, nt, cur = _gather_args(segs, notes, cursor)
    check(_lib.lib().clv_gather_rows_multi(rows, _ptr(idx), int(row0), n, src, u8, out, re, ch, ld, st, of, tb, nt, cur, _stream()),
          "clv_gather_rows_multi")


class TransposeDraw(C.Structure):
    """clv_transpose_draw (include/clvae.h)."""
    _fields_ = [("allowed", C.c_void_p), ("class_map", C.c_void_p),
                ("K", C.c_int32), ("C", C.c_int32), ("D", C.c_int32), ("label_seg", C.c_int32),
                ("seed", C.c_uint64), ("first_row", C.c_uint64), ("step", C.c_uint32),
                ("step_dev", C.c_void_p), ("shift_out", C.c_void_p)]


def gather_transposed(rows, idx, segs, allowed, class_map, K, D, seed, step=0, step_dev=None, first_row=0, shift_out=None,
                      label_seg=None, row0=0, notes=None, cursor=None):
    """gather_rows_multi with a random transposition per output row: segs, idx, row0, notes and cursor as
    there; every segment is a uint8 source of frames of D bytes (float or uint8 output) but segs[label_seg], the float labels
    [*, C].  allowed: uint32 [n] per SOURCE row, bit j = shift j - K allowed; class_map: int32 [(2K+1) * C]; the shift of output
    row r is drawn from the Philox uniform of (seed, step or *step_dev, TRANSPOSE_STREAM, first_row + r) and written to
    shift_out (int32 [rows], optional)."""
    n, src, u8, out, re, ch, ld, st, of, tb, nt, cur = _gather_args(segs, notes, cursor)
    n_cls = int(segs[label_seg][2]) if label_seg is not None else int(class_map.numel()) // (2 * int(K) + 1)
    draw = TransposeDraw(_ptr(allowed), _ptr(class_map), int(K), n_cls, int(D), -1 if label_seg is None else int(label_seg),
                         int(seed) & (2 ** 64 - 1), int(first_row), int(step) & 0xFFFFFFFF, _ptr(step_dev), _ptr(shift_out))
    check(_lib.lib().clv_gather_transposed(rows, _ptr(idx), int(row0), n, src, u8, out, re, ch, ld, st, of, tb, nt, cur,
                                           C.byref(draw), _stream()), "clv_gather_transposed")


def philox_normal2(out0, n0, stream0, first0, out1, n1, stream1, first1, seed, step=0, step_dev=None):
    check(_lib.lib().clv_philox_normal2(_ptr(out0), n0, stream0, first0, _ptr(out1), n1, stream1, first1, seed, step,
                                        _ptr(step_dev), _stream()), "clv_philox_normal2")


def philox_normal(out, n, seed, step=0, stream_id=0, first_index=0, step_dev=None):
    check(_lib.lib().clv_philox_normal(_ptr(out), n, seed, step, _ptr(step_dev), stream_id, first_index, _stream()),
          "clv_philox_normal")


def philox_uniform(out, n, seed, step=0, stream_id=0, first_index=0, step_dev=None):
    check(_lib.lib().clv_philox_uniform(_ptr(out), n, seed, step, _ptr(step_dev), stream_id, first_index, _stream()),
          "clv_philox_uniform")


def act_grad(n, act, y, dy, dpre):
    check(_lib.lib().clv_act_grad(n, act, _ptr(y), _ptr(dy), _ptr(dpre), _stream()), "clv_act_grad")


def i32_add(counter, v=1):
    check(_lib.lib().clv_i32_add(_ptr(counter), int(v), _stream()), "clv_i32_add")


def iw_accumulate(R, T, L, C1, rownll, zargs, eps_z, wargs, eps_w, w_log_var_prior, nvalid, state, step_dev=None):
    """clv_iw_accumulate: fold one importance sample of rows < nvalid into the fp64 state [R, 4]; step_dev (device int32,
    optional) is advanced by one after the launch's work."""
    check(_lib.lib().clv_iw_accumulate(int(R), int(T), int(L), int(C1), _ptr(rownll), _ptr(zargs), _ptr(eps_z),
                                       _ptr(wargs) if C1 else None, _ptr(eps_w) if C1 else None, float(w_log_var_prior),
                                       int(nvalid), _ptr(state), _ptr(step_dev), _stream()), "clv_iw_accumulate")


def iw_finish(R, nvalid, K, state, log_p, elbo, ess):
    """clv_iw_finish: per-window log_p, elbo, ess (fp64 [>= nvalid]) from the state after K samples."""
    check(_lib.lib().clv_iw_finish(int(R), int(nvalid), int(K), _ptr(state), _ptr(log_p), _ptr(elbo), _ptr(ess), _stream()),
          "clv_iw_finish")


def dropout_rows(R, T, n, X, ldx, U, ldu, rate, out, ldo, beta=0.0):
    """out[r, :n] = beta * out + X[r, :n] * mask(U[r // T, :n]), mask(u) = (u >= rate) / (1 - rate) (clv_dropout_rows)."""
    check(_lib.lib().clv_dropout_rows(R, T, n, _ptr(X), ldx, _ptr(U), ldu, float(rate), float(beta), _ptr(out), ldo, _stream()),
          "clv_dropout_rows")


def sigmoid_temper(n, a, inv_temperature):
    """a[:n] = sigmoid(fl32(a * inv_temperature)) in place: the output head of a tempered frame chain (clv_sigmoid_temper)"""
    check(_lib.lib().clv_sigmoid_temper(n, _ptr(a), float(inv_temperature), _stream()), "clv_sigmoid_temper")


def scale_temper(n, eps, z_temperature):
    """eps[:n] = fl32(z_temperature * eps) in place: the latent noise of a tempered frame chain (clv_scale_temper)"""
    check(_lib.lib().clv_scale_temper(n, _ptr(eps), float(z_temperature), _stream()), "clv_scale_temper")


def bernoulli_sample(n, p, u, x):
    check(_lib.lib().clv_bernoulli_sample(n, _ptr(p), _ptr(u), _ptr(x), _stream()), "clv_bernoulli_sample")


def bernoulli_sample_clamped(n, D, nsteps, S, p, u, clamp, step_dev, x):
    """bernoulli_sample under the constraint roll clamp [n/D, nsteps, D] (uint8): row *step_dev - S, none before step S."""
    check(_lib.lib().clv_bernoulli_sample_clamped(n, D, nsteps, S, _ptr(p), _ptr(u), _ptr(clamp), _ptr(step_dev), _ptr(x),
                                                  _stream()), "clv_bernoulli_sample_clamped")


def smc_sample(R, D, P, nsteps, S, p, u, clamp, step_dev, x, ell, hist):
    """particle rows r < R (P per melody): x = clamped Bernoulli draw of p with roll row r // P of clamp [R/P, nsteps, D]
    at step *step_dev - S; ell [R] fp64 = the frame's log weight increment; hist [nsteps, R, D] uint8."""
    check(_lib.lib().clv_smc_sample(R, D, P, nsteps, S, _ptr(p), _ptr(u), _ptr(clamp), _ptr(step_dev), _ptr(x), _ptr(ell),
                                    _ptr(hist), _stream()), "clv_smc_sample")


def bernoulli_sample_voices(n, D, nsteps, S, p, u, clamp, voices, step_dev, x, logb=None):
    """bernoulli_sample_clamped given each frame's voice count: voices [n/D, nsteps, 2] uint8 holds (lo, hi)
    per returned frame, (0, 255) = free; clamp (the roll) may be None; logb [n/D] fp64 (optional) = log P(count in range)."""
    check(_lib.lib().clv_bernoulli_sample_voices(n, D, nsteps, S, _ptr(p), _ptr(u), _ptr(clamp), _ptr(voices), _ptr(step_dev),
                                                 _ptr(x), _ptr(logb), _stream()), "clv_bernoulli_sample_voices")


def smc_sample_voices(R, D, P, nsteps, S, p, u, clamp, voices, step_dev, x, ell, hist, logb=None):
    """smc_sample given each frame's voice count: voices [R/P, nsteps, 2] uint8 per melody, as the roll (which
    may be None); ell gains log P(count in range | forced notes), which logb [R] fp64 (optional) also receives."""
    check(_lib.lib().clv_smc_sample_voices(R, D, P, nsteps, S, _ptr(p), _ptr(u), _ptr(clamp), _ptr(voices), _ptr(step_dev),
                                           _ptr(x), _ptr(ell), _ptr(hist), _ptr(logb), _stream()), "clv_smc_sample_voices")


def smc_resample(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc, step_dev):
    """per melody m < G: log Z, normalized log weights, ESS [G, nsteps], systematic resampling below tau * P, ancestors
    anc [nsteps, G*P] of step *step_dev - S; m0 = global index of melody 0 (the resampling uniform's Philox index)."""
    check(_lib.lib().clv_smc_resample(G, P, nsteps, S, int(seed), int(m0), float(tau), _ptr(ell), _ptr(logW), _ptr(logZ),
                                      _ptr(ess), _ptr(nres), _ptr(flag), _ptr(anc), _ptr(step_dev), _stream()),
          "clv_smc_resample")


def smc_resample_carry(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc, step_dev, t0, carry):
    """smc_resample of a filter stream: the resampling uniform's Philox step is t0 + *step_dev, and with
    carry step 0 continues logW, logZ and nres instead of starting them.  t0 = 0, carry = False: smc_resample."""
    check(_lib.lib().clv_smc_resample_carry(G, P, nsteps, S, int(seed), int(m0), float(tau), _ptr(ell), _ptr(logW),
                                            _ptr(logZ), _ptr(ess), _ptr(nres), _ptr(flag), _ptr(anc), _ptr(step_dev),
                                            int(t0), int(bool(carry)), _stream()), "clv_smc_resample_carry")


def smc_commit(G, P, D, n, anc, hist, cap, pend_anc, pend_hist, head, length, out_cap, ncommit, out):
    """after a chunk of n filter steps (anc [n, G*P] int32, hist [n, G*P, D] uint8): per melody the prefix of its pending
    steps -- the ring pend_anc [cap, G*P], pend_hist [cap, G*P, D], head, length [G] int32, then the chunk -- through which
    all P lineages pass by one row goes to out [G, out_cap, D] uint8 and leaves the ring, ncommit [G] int32 frames; the
    rest of the chunk joins the ring.  The caller keeps length + n <= min(cap, out_cap) (else ncommit = -1)."""
    check(_lib.lib().clv_smc_commit(G, P, D, n, _ptr(anc), _ptr(hist), int(cap), _ptr(pend_anc), _ptr(pend_hist), _ptr(head),
                                    _ptr(length), int(out_cap), _ptr(ncommit), _ptr(out), _stream()), "clv_smc_commit")


def smc_collapse(G, P, D, seed, m0, step, final, pick_of, logW, cap, pend_anc, pend_hist, head, length, out_cap, picks, out,
                 anc_row=None, flag=None):
    """per melody with pick_of != 0 (None: all): picks [G] int32 = one particle drawn from logW (Philox stream 0xFFFFFFF8,
    step `step`, index m0 + m), its pending lineage to out [G, out_cap, D] uint8, anc_row [G*P] / flag [G] for SmcGather,
    logW = -log P, length = 0.  final: the terminal draw of smc_backtrack (its stream); only picks and out are written."""
    check(_lib.lib().clv_smc_collapse(G, P, D, int(seed), int(m0), int(step), int(bool(final)), _ptr(pick_of), _ptr(logW),
                                      int(cap), _ptr(pend_anc), _ptr(pend_hist), _ptr(head), _ptr(length), int(out_cap),
                                      _ptr(picks), _ptr(out), _ptr(anc_row), _ptr(flag), _stream()), "clv_smc_collapse")


class SmcGather:
    """clv_smc_gather over a fixed list of fp32 [R, width] buffers: the pointer list lives on the host (the launch copies
    it into its arguments, so a captured graph keeps it) and the scratch buffer is allocated once."""

    def __init__(self, R, P, nsteps, S, bufs):
        self.R, self.P, self.nsteps, self.S = int(R), int(P), int(nsteps), int(S)
        widths = [int(b.numel()) // self.R for b in bufs]
        if any(w * self.R != b.numel() or not b.is_contiguous() or b.dtype != torch.float32 for w, b in zip(widths, bufs)):
            raise ValueError("smc gather buffers must be contiguous float32 [R, width]")
        self.bufs = list(bufs)
        self._ptrs = (C.c_void_p * len(bufs))(*[b.data_ptr() for b in bufs])
        self._widths = (C.c_int * len(bufs))(*widths)
        self.scratch = torch.empty(sum(widths) * self.R, dtype=torch.float32, device=bufs[0].device)

    def __call__(self, anc, flag, step_dev):
        check(_lib.lib().clv_smc_gather(self.R, self.P, self.nsteps, self.S, len(self.bufs), C.cast(self._ptrs, C.c_void_p),
                                        C.cast(self._widths, C.c_void_p), _ptr(self.scratch), _ptr(anc), _ptr(flag),
                                        _ptr(step_dev), _stream()), "clv_smc_gather")


def smc_backtrack(G, P, nsteps, D, n_out, seed, m0, step, logW, anc, hist, Xs, picks=None):
    """n_out draws per melody from the final weights (Philox uniform at `step`, index m0 + m), lineage walked back through
    anc: Xs [G, n_out, nsteps, D] fp32; picks [G, n_out] int32 (optional) = the drawn final particles."""
    check(_lib.lib().clv_smc_backtrack(G, P, nsteps, D, n_out, int(seed), int(m0), int(step), _ptr(logW), _ptr(anc),
                                       _ptr(hist), _ptr(Xs), _ptr(picks), _stream()), "clv_smc_backtrack")


SMC_W_CATEGORICAL, SMC_W_LOGISTIC_NORMAL = 0, 1


def smc_init_w(G, P, Cn, mode, seed, m0, probs, mean, log_var, wr):
    """the label rows wr [G*P, Cn] of G melodies x P particles from their key prior: mode SMC_W_CATEGORICAL
    with probs [G, Cn] fp64 (a systematic draw of P keys, one-hot rows), SMC_W_LOGISTIC_NORMAL with mean, log_var
    [G, Cn-1] fp32; m0 = global index of melody 0 (the Philox indices follow the global melody / row)."""
    check(_lib.lib().clv_smc_init_w(G, P, Cn, int(mode), int(seed), int(m0), _ptr(probs), _ptr(mean), _ptr(log_var), _ptr(wr),
                                    _stream()), "clv_smc_init_w")


def smc_w_posterior(G, P, Cn, nsteps, S, logW, wr, step_dev, out):
    """out[m, k] = sum_p exp(logW) * wr rows of melody m at step k = *step_dev - S (out [G, nsteps, Cn] fp64); runs in the
    frame after the gather, and does nothing on the seed steps and the bridge."""
    check(_lib.lib().clv_smc_w_posterior(G, P, Cn, nsteps, S, _ptr(logW), _ptr(wr), _ptr(step_dev), _ptr(out), _stream()),
          "clv_smc_w_posterior")


def smc_take_w(G, P, Cn, n_out, picks, wr, w_out):
    """w_out [G, n_out, Cn] = the label rows of the particles picks [G, n_out] that smc_backtrack drew"""
    check(_lib.lib().clv_smc_take_w(G, P, Cn, n_out, _ptr(picks), _ptr(wr), _ptr(w_out), _stream()), "clv_smc_take_w")


def smc_pin_z(G, P, L, T, z_ref, step_dev, z):
    """a conditional sweep's latent pin: z[m*P] = z_ref[m, *step_dev] of z_ref [G, T, L]; z [G*P, L]"""
    check(_lib.lib().clv_smc_pin_z(G, P, L, T, _ptr(z_ref), _ptr(step_dev), _ptr(z), _stream()), "clv_smc_pin_z")


def smc_pin_frame(G, P, D, nsteps, S, x_ref, bridge, step_dev, x, hist):
    """a conditional sweep's frame pin: at returned step k = *step_dev - S, x[m*P] and hist[k, m*P] = x_ref[m, k] (x_ref
    [G, nsteps, D] uint8); at step S - 1 (S > 0) x[m*P] = bridge[m] (bridge [G, D] fp32 or None)"""
    check(_lib.lib().clv_smc_pin_frame(G, P, D, nsteps, S, _ptr(x_ref), _ptr(bridge), _ptr(step_dev), _ptr(x), _ptr(hist),
                                       _stream()), "clv_smc_pin_frame")


def smc_resample_conditional(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc, step_dev):
    """smc_resample with conditional multinomial resampling: row m*P keeps itself, every other particle draws its own
    uniform (stream GIBBS_STREAM, index = its global row)"""
    check(_lib.lib().clv_smc_resample_conditional(G, P, nsteps, S, int(seed), int(m0), float(tau), _ptr(ell), _ptr(logW),
                                                  _ptr(logZ), _ptr(ess), _ptr(nres), _ptr(flag), _ptr(anc), _ptr(step_dev),
                                                  _stream()), "clv_smc_resample_conditional")


def smc_backtrack_path(G, P, nsteps, S, D, L, picks, anc, hist, zhist, bridge_rows, x_ref, z_ref, bridge_ref, renewed):
    """the lineage of particle picks [G] as the next retained path: x_ref [G, nsteps, D] uint8, z_ref [G, S+nsteps, L] from
    zhist [S+nsteps, G*P, L], bridge_ref [G, D] from bridge_rows [G*P, D] (both None without seed steps), renewed
    [G, nsteps] uint8 = frame k did not come from the pinned row"""
    check(_lib.lib().clv_smc_backtrack_path(G, P, nsteps, S, D, L, _ptr(picks), _ptr(anc), _ptr(hist), _ptr(zhist),
                                            _ptr(bridge_rows), _ptr(x_ref), _ptr(z_ref), _ptr(bridge_ref), _ptr(renewed),
                                            _stream()), "clv_smc_backtrack_path")


def key_track_windows(N, T, D, Hd, Cn, hop, K, frames, piece_off, win_off, Kh, bh, Ka, ba, seed, piece0, wargs, logp):
    """the label head on every window of N pieces of the uint8 roll frames [F, D] (clv_key_track_windows):
    window j of piece n starts at frame j * hop and goes to row win_off[n] + j of wargs [Wtot, 2(Cn-1)] and logp [Wtot, Cn];
    piece_off, win_off int64 [N+1] on the device; K = 0 the noise-free label, K >= 1 the mean over K label samples."""
    check(_lib.lib().clv_key_track_windows(int(N), int(T), int(D), int(Hd), int(Cn), int(hop), int(K), _ptr(frames),
                                           _ptr(piece_off), _ptr(win_off), _ptr(Kh), _ptr(bh), _ptr(Ka), _ptr(ba), int(seed),
                                           int(piece0), _ptr(wargs), _ptr(logp), _stream()), "clv_key_track_windows")


def key_track_smooth(N, Cn, win_off, logp, log_prior, log_trans, kappa, post, path, log_evidence, piece_post):
    """forward-backward and Viterbi over the rows win_off[n] .. win_off[n+1] of logp [Wtot, Cn] per piece, in fp64
    (clv_key_track_smooth): post [Wtot, Cn], path [Wtot] int32, log_evidence [N], piece_post [N, Cn]; log_prior [Cn] fp64
    or None (uniform), log_trans [Cn, Cn] fp64 (row = from), 0 < kappa <= 1."""
    check(_lib.lib().clv_key_track_smooth(int(N), int(Cn), _ptr(win_off), _ptr(logp), _ptr(log_prior), _ptr(log_trans),
                                          float(kappa), _ptr(post), _ptr(path), _ptr(log_evidence), _ptr(piece_post),
                                          _stream()), "clv_key_track_smooth")


def roll_nearest_workspace_bytes(Fq, Fc, Wq):
    return int(_lib.lib().clv_roll_nearest_workspace_bytes(int(Fq), int(Fc), int(Wq)))


def roll_nearest(Nq, Nc, W, hop, S, D, Fq, Fc, Wq, q_roll, q_off, c_roll, c_off, qwin_off, exclude, dist, shift, cframe,
                 workspace=None):
    """the nearest corpus window of every query window (clv_roll_nearest): q_roll [>= Fq, D], c_roll [>= Fc, D]
    uint8 0/1; q_off [Nq+1], c_off [Nc+1], qwin_off [Nq+1] int64 on the device, their last entries Fq, Fc, Wq; exclude [Nq]
    int32 or None; dist, shift [>= Wq] int32 and cframe [>= Wq] int64 receive (dist, s, global corpus frame) of the smallest
    (dist, rank(s), frame), or (-1, 0, -1).  workspace: a uint8 tensor of roll_nearest_workspace_bytes(Fq, Fc, Wq) bytes,
    or None to allocate one; it is returned."""
    Fq, Fc, Wq = int(Fq), int(Fc), int(Wq)
    if Fq > q_roll.shape[0] or Fc > c_roll.shape[0] or Wq > min(dist.numel(), shift.numel(), cframe.numel()):
        raise _lib.ClvError("roll_nearest: Fq, Fc or Wq name more rows than the tensors hold")
    if workspace is None:
        workspace = torch.empty(max(roll_nearest_workspace_bytes(Fq, Fc, Wq), 16), dtype=torch.uint8, device=q_roll.device)
    check(_lib.lib().clv_roll_nearest(int(Nq), int(Nc), int(W), int(hop), int(S), int(D), Fq, Fc, Wq, _ptr(q_roll), _ptr(q_off),
                                      _ptr(c_roll), _ptr(c_off), _ptr(qwin_off), _ptr(exclude), _ptr(workspace),
                                      int(workspace.numel()), _ptr(dist), _ptr(shift), _ptr(cframe), _stream()),
          "clv_roll_nearest")
    return workspace


def roll_stats_columns(D, Lmax):
    """S, the columns of one piece's row of roll_stats' table (clv_roll_stats_column_count); 0 for D outside 1..116 or Lmax
    outside 1..64"""
    return int(_lib.lib().clv_roll_stats_column_count(int(D), int(Lmax)))


def roll_stats(N, D, Lmax, low, F, roll, off, tonic, table):
    """the texture histograms of N pieces (clv_roll_stats): roll [>= F, D] uint8, any non-zero byte a sounding
    note; off [N+1] int64 on the device, off[0] = 0, off[N] = F; tonic [N] int32 (0..11, -1: unknown, counted as 0) or
    None; low the MIDI number of note 0; table [>= N, roll_stats_columns(D, Lmax)] int64 is overwritten with the sections
    pitch, degree, voices, interval, duration, change, top_step, bottom_step, span of every piece."""
    N, F = int(N), int(F)
    S = roll_stats_columns(D, Lmax)
    if F > (roll.shape[0] if roll is not None else 0) or off.numel() < N + 1 or table.numel() < N * S \
            or (tonic is not None and tonic.numel() < N):
        raise _lib.ClvError("roll_stats: N or F name more rows than the tensors hold")
    check(_lib.lib().clv_roll_stats(N, int(D), int(Lmax), int(low), F, _ptr(roll), _ptr(off), _ptr(tonic), _ptr(table),
                                    _stream()), "clv_roll_stats")


class Graph:
    """Capture the kernels enqueued inside the ``with`` block on the current stream; replay with launch()."""

    def __init__(self):
        self.handle = C.c_void_p()
        self._stream = None

    def __enter__(self):
        self._stream = torch.cuda.Stream()
        self._stream.wait_stream(torch.cuda.current_stream())
        self._ctx = torch.cuda.stream(self._stream)
        self._ctx.__enter__()
        check(_lib.lib().clv_graph_begin_capture(_stream()), "graph begin")
        return self

    def __exit__(self, et, ev, tb):
        code = _lib.lib().clv_graph_end_capture(_stream(), C.byref(self.handle))
        self._ctx.__exit__(et, ev, tb)
        torch.cuda.current_stream().wait_stream(self._stream)
        if et is None:
            check(code, "graph end")
        return False

    def launch(self):
        check(_lib.lib().clv_graph_launch(self.handle, _stream()), "graph launch")

    def __del__(self):
        try:
            if self.handle:
                _lib.lib().clv_graph_destroy(self.handle)
        except Exception:
            pass


def prof_enable(on=True):
    check(_lib.lib().clv_prof_enable(int(on)))


def prof_empty_scope():
    """an empty bracket of the profiler's events on the current stream (record name "event_pair")"""
    check(_lib.lib().clv_prof_empty_scope(_stream()))


def prof_collect(cap=64):
    arr = (_lib.ProfRecord * cap)()
    n = _lib.lib().clv_prof_collect(arr, cap)
    if n < 0:
        check(n, "clv_prof_collect")
    return [(arr[i].name.decode(), arr[i].launches, arr[i].total_ms) for i in range(n)]
