"""-m gpu: the edges of the kernel-gradient product's loader (csrc/wgrad_bf16.hip), single and pair entry.

The producers read every operand through a buffer descriptor that covers exactly a workgroup's row range, request stages
beyond the range like any other (no load sits behind a condition) and rely on the range check for: the rows of a ragged
last stage, whole stages beyond the range, the H row in front of row 0, an absent Z.  So every operand here is a VIEW into
a larger allocation that is NaN (bytes: 255) everywhere else, with 64 guard rows on either side: a read outside [0, K)
shows as a NaN (a wrong sum) in an output.  Outputs are pre-filled with a sentinel, every launch runs twice and must
reproduce bit for bit, and the bar against fp64 numpy is the project's 2e-6 x sum|a.b| (tests/test_gpu_ops.py).

Row counts: 31 ... 160 give workgroups of ONE stage each (a row range is at least 32 rows: 1 ... 5 workgroups, full and
ragged); the counts above them are the smallest that give a workgroup 2, 3, 4 and 5 stages (128 row ranges in the single
launch, 64 in the pair's, times split_scale), with a ragged last range: odd and even stage counts of the two-set pipeline.
Window lengths: 16 (starts at rows 0 and 16 of a stage: the select path), 5 and 7 (starts anywhere: the division path),
K (one window)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, NX, GUARD = 352, 88, 64
K_ONE_STAGE = [31, 32, 33, 64, 65, 97, 160]
K_SINGLE = K_ONE_STAGE + [4225, 8225, 12353, 16513]        # 128 ranges of 64 / 96 / 128 / 160 rows, the last one ragged
K_PAIR = K_ONE_STAGE + [2113, 4161, 6209, 8257]            # 64 ranges of the same lengths
WINDOWS = [16, 5, 7, 0]                                    # 0: K
NZS = [0, 2, 8, 32]
FRAMES = ['u8', 'exact', 'general']
NHS = [88, 64, 96]


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def guarded(a, dev):
    """The device copy of `a` as rows [GUARD, GUARD + K) of an allocation that is NaN (255 for bytes) everywhere else."""
    a = np.ascontiguousarray(a)
    big = np.full((a.shape[0] + 2 * GUARD,) + a.shape[1:], 255 if a.dtype == np.uint8 else np.nan, a.dtype)
    big[GUARD:GUARD + a.shape[0]] = a
    return torch.as_tensor(big, device=dev)[GUARD:GUARD + a.shape[0]]


class Problem:
    """One LSTM's operands (host and guarded device copies), its outputs and its fp64 references."""

    def __init__(self, dev, rng, K, Tn, nz, frames, nh):
        self.K, self.Tn, self.nz, self.nh, self.frames = K, Tn, nz, nh, frames
        X = (rng.random((K, NX)) < 0.0443) if frames != 'general' else rng.standard_normal((K, NX))
        X = X.astype(np.uint8 if frames == 'u8' else np.float32)
        self.ldz = max(nz, 1) + 3                      # the latent columns in a buffer of their own, rows longer than nz
        Z = rng.standard_normal((K, self.ldz)).astype(np.float32)
        hs = np.tanh(rng.standard_normal((K, nh))).astype(np.float32)
        dz = (rng.standard_normal((K, N)) * np.exp(rng.standard_normal((K, 1)) * 2)).astype(np.float32)
        Hs = np.zeros_like(hs)                         # H'_k = h of the previous step, zero at window starts
        Hs[1:] = hs[:-1]
        Hs[::Tn] = 0
        self.dX, self.dZ, self.dH, self.ddz = guarded(X, dev), guarded(Z, dev), guarded(hs, dev), guarded(dz, dev)
        f8 = lambda a: a.astype(np.float64)
        self.refs = [(f8(A).T @ f8(dz), np.abs(f8(A)).T @ np.abs(f8(dz)) + 1e-30)
                     for A in (X, Hs) + ((Z[:, :nz],) if nz else ())]
        self.dev = dev

    def outputs(self):
        s = lambda r: torch.full((r, N), -5.0, dtype=torch.float32, device=self.dev)
        return [s(NX), s(self.nh)] + ([s(self.nz)] if self.nz else [])

    def args(self, out):
        """the argument tuple of ops.lstm_wgrad up to dKz"""
        return (self.K, N, self.dX, NX, NX, self.frames != 'general', self.dH, self.nh, self.nh, self.Tn,
                self.dZ if self.nz else None, self.ldz, self.nz, self.ddz, out[0], out[1], out[2] if self.nz else None)

    def check(self, runs, what):
        for a, b in zip(*runs):
            assert torch.equal(a, b), what + ": two launches differ"
        for got, (ref, mag) in zip(runs[0], self.refs):
            g = got.cpu().numpy()
            assert np.isfinite(g).all(), what + ": a read outside the operand's rows"
            err = (np.abs(g - ref) / mag).max()
            assert err < 2e-6, (what, err)


def frames_for(ops, nh, nz, frames):
    """general float frames where the kernel takes them (not in its wide form), exact ones otherwise"""
    return frames if frames != 'general' or ops.lstm_wgrad_supported(N, NX, nh, nz, False) else 'exact'


def single_cases():
    """every K with four combinations of the other parameters, each list walked at its own stride: every value of every
    list meets every kind of K (one stage, several) several times"""
    out = []
    for i, K in enumerate(K_SINGLE):
        for j in range(4):
            n = 4 * i + j
            out.append((K, WINDOWS[(i + j) % 4], NZS[(n // 2 + j) % 4], FRAMES[n % 3], NHS[(n // 3) % 3], 1 + (i + j // 2) % 2, j % 2 == 1))
    return out


@pytest.mark.parametrize("K,Tn,nz,frames,nh,scale,defer", single_cases())
def test_single_launch_edges(dev, K, Tn, nz, frames, nh, scale, defer):
    from clvae_amd import ops
    Tn = Tn or K
    frames = frames_for(ops, nh, nz, frames)
    assert ops.lstm_wgrad_supported(N, NX, nh, nz, frames != 'general')
    p = Problem(dev, np.random.default_rng([K, Tn, nz, nh]), K, Tn, nz, frames, nh)
    runs = []
    for rep in range(2):
        out = p.outputs()
        rq = ops.ReduceQueue(dev) if defer else None
        ops.lstm_wgrad(*p.args(out), ops.Workspace(dev), defer=rq, split_scale=scale)
        if rq is not None:
            rq.flush()
        torch.cuda.synchronize()
        runs.append(out)
    p.check(runs, "K %d window %d nz %d %s nh %d scale %d" % (K, Tn, nz, frames, nh, scale))


def pair_cases():
    out = []
    for i, K in enumerate(K_PAIR):
        for j in range(2):
            n = 2 * i + j
            nzs = [(0, 2), (0, 8), (32, 32), (0, 0), (2, 8)][n % 5]          # the two problems take the same form of the kernel
            out.append((K, WINDOWS[(i + 2 * j + 1) % 4], nzs, FRAMES[(n + 1) % 3], NHS[0] if nzs != (32, 32) else NHS[n % 3],
                        1 + (i + j) % 2, n % 3 == 0))
    return out


@pytest.mark.parametrize("K,Tn,nzs,frames,nh,scale,defer", pair_cases())
def test_pair_launch_edges(dev, K, Tn, nzs, frames, nh, scale, defer):
    from clvae_amd import ops
    Tn = Tn or K
    frames = frames_for(ops, nh, max(nzs), frames)
    rng = np.random.default_rng([K, Tn, nzs[0], nzs[1], nh])
    ps = [Problem(dev, rng, K, Tn, nz, frames, nh) for nz in nzs]
    outs0 = [p.outputs() for p in ps]
    assert ops.lstm_wgrad_pair_supported(ps[0].args(outs0[0]), ps[1].args(outs0[1]))
    runs = [[], []]
    for rep in range(2):
        outs = [p.outputs() for p in ps]
        rq = ops.ReduceQueue(dev) if defer else None
        ops.lstm_wgrad_pair(ps[0].args(outs[0]), ps[1].args(outs[1]), (ops.Workspace(dev), ops.Workspace(dev)), defer=rq,
                            split_scale=scale)
        if rq is not None:
            rq.flush()
        torch.cuda.synchronize()
        for r, o in zip(runs, outs):
            r.append(o)
    for p, r in zip(ps, runs):
        p.check(r, "pair K %d window %d nz %d (of %s) %s nh %d scale %d" % (K, Tn, p.nz, nzs, frames, nh, scale))


def test_operands_of_two_gib_are_refused_before_any_launch(dev):
    """The descriptors' offsets are 32 bits wide: (K + 160) rows of an operand at 2 GiB or more are refused by the host
    code (include/clvae.h) -- the query says so, the entry points return an error, nothing is launched (the sentinels stay)."""
    from clvae_amd import ops
    K = 64
    p = Problem(dev, np.random.default_rng(0), K, 16, 2, 'exact', 88)
    assert ops.lstm_wgrad_rows_supported(K, N, p.dX, NX, True, 88, p.ldz, 2)
    rows = (1 << 31) // (N * 4)                                 # the most rows of dz below 2 GiB
    assert ops.lstm_wgrad_rows_supported(rows - 160, N, p.dX, NX, True, 88, p.ldz, 2)
    assert not ops.lstm_wgrad_rows_supported(rows - 159, N, p.dX, NX, True, 88, p.ldz, 2)
    big = (1 << 31) // ((K + 160) * 4) // 4 * 4 + 4             # a row stride (floats) that puts K + 160 rows at 2 GiB
    assert not ops.lstm_wgrad_rows_supported(K, N, p.dX, NX, True, big, p.ldz, 2)
    assert not ops.lstm_wgrad_rows_supported(K, N, p.dX, NX, True, 88, big, 2)
    assert ops.lstm_wgrad_rows_supported(K, N, p.dX, NX, True, 88, big, 0)                 # an absent Z has no stride
    assert not ops.lstm_wgrad_rows_supported(K, N, p.dX, big, True, 88, p.ldz, 2)          # float frames: 4 bytes each
    assert ops.lstm_wgrad_rows_supported(K, N, guarded(np.zeros((K, NX), np.uint8), dev), big, True, 88, p.ldz, 2)   # bytes: 1
    out = p.outputs()
    a = list(p.args(out))
    a[7] = big                                                  # ldh
    with pytest.raises(RuntimeError):
        ops.lstm_wgrad(*a, ops.Workspace(dev))
    assert not ops.lstm_wgrad_pair_supported(tuple(a), p.args(out))
    torch.cuda.synchronize()
    for o in out:
        assert bool((o == -5.0).all())
