"""-m gpu: every public device sampling call of both families on both routes launches what it launched, and returns what it
returned, before the two families' vary / decode_latents / generate_smc became one body each (engine_generate._Generate).
Per case: the profiler's launch list (names and counts) and the SHA-256 of every returned tensor, compared for equality with
tests/golden/sampling_routes.json, which record_cases() wrote on the MI355X from the commit before that change.  The samplers
draw Philox noise and sum in a fixed order, so there is no tolerance.  The frame chain runs eagerly under the profiler (every
frame's launches are counted) and once more captured, which must give the same tensors."""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_clamped_generation as TC

pytestmark = pytest.mark.gpu

N, S, T, D, C, B, SEED = 3, 2, 5, 88, 4, 8, 97
L = {'cl_vae': 3, 'cl_vrnn': 2}
SMC_N, SMC_P = 2, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampling_routes.json")

ROUTED = ('generate', 'generate_roll', 'generate_tempered', 'generate_resumed', 'vary_own', 'vary_source', 'vary_zout',
          'decode_own', 'decode_history_noise_rows')
CHAIN_ONLY = ('smc_w', 'smc_w_prior')           # the filter has the frame chain only
CASES = tuple("%s/%s/%s" % (k, r, c) for k in ('cl_vae', 'cl_vrnn') for r in ('persistent', 'chain') for c in ROUTED) \
    + tuple("%s/chain/%s" % (k, c) for k in ('cl_vae', 'cl_vrnn') for c in CHAIN_ONLY)
SKIPPED = ()                                    # cases the recording commit itself did not reproduce run to run: none


def _sha(t):
    a = t.detach().cpu().contiguous().numpy()
    return "%s%s:%s" % (a.dtype, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def _digests(out):
    """name -> digest of every tensor in a call's outputs (a dict of tensors, GenStates and Smc results)"""
    d = {}
    for k, v in out.items():
        if isinstance(v, torch.Tensor):
            d[k] = _sha(v)
        elif hasattr(v, '_fields'):
            d.update({"%s.%s" % (k, f): _sha(getattr(v, f)) for f in v._fields})
        else:                                   # a GenState
            d[k + ".t"] = int(v.t)
            d.update({"%s.%s" % (k, f): _sha(x) for f, x in v.tensors().items()})
    return d


def _engine(dev, kind):
    if kind == 'cl_vae':
        return TC._vae(dev, L=L[kind], C=C, B=B)
    return TC._vrnn(dev, L[kind], Cn=C, B=B)


def _calls(eng, kind, dev):
    """case name -> f(**route) that makes the call and returns its outputs by name"""
    from clvae_amd.engine_generate import WPrior
    rng = np.random.default_rng(11)
    Lk = L[kind]
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    x_seed, w = TC._inputs(dev, N, S if kind == 'cl_vrnn' else None, C, 3)
    roll = TC._roll(N, T, seed=5)
    sources = t(rng.random((N, T, D)) < 0.06)
    x0 = t(rng.random((N, D)) < 0.06)
    hist = t(rng.random((N, T, D)) < 0.06)
    w2 = t(np.eye(C)[rng.integers(0, C, N)])
    z = t(rng.standard_normal((N, T, Lk)))
    xs_smc, w_smc = TC._inputs(dev, SMC_N, S if kind == 'cl_vrnn' else None, C, 4)
    roll_smc = TC._roll(SMC_N, T, seed=6)
    new = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)

    def resumed(**r):
        Xa, sa = eng.generate(x_seed, w, 2, seed=SEED, return_state=True, **r)
        Xb, sb = eng.generate(None, w, 3, seed=SEED, state=sa, return_state=True, **r)
        return dict(Xa=Xa, state_a=sa, Xb=Xb, state_b=sb)

    def vary(history, zout=False, **r):
        out = dict(xhat_out=new(N, T, D))
        if zout:
            out['zout'] = new(3, N, T, Lk)
        out['Xs'] = eng.vary(sources, w, w2, x0=x0, history=history, seed=SEED, clamp=roll, **out, **r)
        return out

    def decode(history, noise_rows, **r):
        xh = new(N, T, D)
        return dict(Xs=eng.decode_latents(z, w2, x0=x0, history=history, seed=SEED, noise_rows=noise_rows, xhat_out=xh, **r),
                    xhat_out=xh)

    def smc(use_graph=True, **kw):
        return dict(r=eng.generate_smc(xs_smc, kw.pop('w', None), T, roll_smc, SMC_P, n_out=2, seed=SEED, chunk=1,
                                       use_graph=use_graph, **kw))

    return {
        'generate': lambda **r: dict(Xs=eng.generate(x_seed, w, T, seed=SEED, **r)),
        'generate_roll': lambda **r: dict(Xs=eng.generate(x_seed, w, T, seed=SEED, clamp=roll, **r)),
        'generate_tempered': lambda **r: dict(Xs=eng.generate(x_seed, w, T, seed=SEED, temperature=0.8, z_temperature=0.5, **r)),
        'generate_resumed': resumed,
        'vary_own': lambda **r: vary('own', **r),
        'vary_source': lambda **r: vary('source', **r),
        'vary_zout': lambda **r: vary('own', zout=True, **r),
        'decode_own': lambda **r: decode('own', None, **r),
        'decode_history_noise_rows': lambda **r: decode(hist, [0, 0, 2], **r),
        'smc_w': lambda **r: smc(w=w_smc, **r),
        'smc_w_prior': lambda **r: smc(w_prior=WPrior.uniform(SMC_N, C), **r),
    }


def run_cases(dev):
    """case id -> {'launches': [[name, count], ...], 'digests': {output: sha256}} for every case of CASES"""
    from clvae_amd import ops
    got = {}
    for kind in ('cl_vae', 'cl_vrnn'):
        eng = _engine(dev, kind)
        calls = _calls(eng, kind, dev)
        for cid in CASES:
            k, route, name = cid.split('/')
            if k != kind:
                continue
            kw = {} if name in CHAIN_ONLY else dict(persistent=route == 'persistent')
            if route == 'chain':
                kw['use_graph'] = False         # eager: the profiler then counts the launches of every frame
            ops.prof_enable(True)
            try:
                out = calls[name](**kw)
                launches = [[n, int(c)] for n, c, _ in ops.prof_collect(cap=256)]
            finally:
                ops.prof_enable(False)          # process-wide: no other module sees it on
            torch.cuda.synchronize()
            digests = _digests(out)
            if route == 'chain':                # the captured chain gives the same tensors
                out = calls[name](**dict(kw, use_graph=True))
                torch.cuda.synchronize()
                assert _digests(out) == digests, cid
            got[cid] = dict(launches=launches, digests=digests)
    return got


def record_cases(path):
    """write the fixture (run on the commit whose behaviour is to be kept)"""
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    got = run_cases(torch.device("cuda:0"))
    with open(path, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    return got


@pytest.fixture(scope="module")
def got():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return run_cases(torch.device("cuda:0"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_every_listed_case(golden):
    assert SKIPPED == ()                        # stays empty unless the recording commit itself was not reproducible
    assert sorted(golden) == sorted(c for c in CASES if c not in SKIPPED)
    for cid, rec in golden.items():
        assert rec['launches'] and rec['digests'], cid


@pytest.mark.parametrize("cid", CASES)
def test_launches_and_results_are_the_recorded_ones(got, golden, cid):
    if cid in SKIPPED:
        return
    assert got[cid]['launches'] == golden[cid]['launches']
    assert got[cid]['digests'] == golden[cid]['digests']
