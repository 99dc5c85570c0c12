"""-m gpu: the pair kernels (csrc/lstm_pair.hip) at the smallest shapes at which the rotation of the backward chains' two
record sets (rA, rB: requested two steps ahead, the loop body is two steps) can go wrong, on the instances configuration 3
runs -- backward <G, ZP = 4, WZG = true>, i.e. latent_dim 1 and 2 with the head gradient on, both gate forms:
  T = 1     only rA is consumed, plus the odd-T extra step (its loads lie beyond the window: zeros)
  T = 2     each set used once, nothing re-requested is consumed
  T = 3     the first re-request (rA of step T-3) is consumed, in the odd-T extra iteration's first half
  T = 5, 6  a set requested in the loop is consumed in the loop, odd and even
B = 1 and 2 (one workgroup, and a second one whose rows lie behind the first's).

Forward and backward against tests/pair_reference.py at test_gpu_pair.py's tolerances (its case builders and checks); dz of
both chains, dzsum, dzargs, dWz and dbz of two backward launches on the same records bit for bit; every buffer NaN-filled
before its launch with canaries behind (helpers.Bufs)."""
import pytest

torch = pytest.importorskip("torch")

import test_gpu_pair as TP
from helpers import Bufs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


@pytest.mark.parametrize("gate", ['hard_sigmoid', 'sigmoid'])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("Tn", [1, 2, 3, 5, 6])
def test_pair_small_windows(dev, Tn, B, L, gate):
    xp_dec = bool((Tn + B) & 1)
    c = TP.make_case(B, Tn, L, gate, xp_dec, 9000 + 100 * Tn + 10 * B + L)
    bufs = Bufs(dev)
    pack = TP.run_pack(c, dev, bufs)
    f = TP.run_fwd(c, dev, bufs, pack)
    torch.cuda.synchronize()
    TP.check_forward(c, f)
    r1 = TP.run_bwd(c, dev, bufs, pack, f)
    r2 = TP.run_bwd(c, dev, bufs, pack, f)
    torch.cuda.synchronize()
    TP.check_backward(c, f, r1)
    TP.check_backward(c, f, r2)
    for k in ('dz_dec', 'dz_enc', 'dzsum_dec', 'dzsum_enc', 'dzargs', 'dWz', 'dbz'):
        assert torch.equal(r1[k], r2[k]), k
        assert not torch.isnan(r1[k]).any(), k
    bufs.check_canaries()
