"""What the twelve entry points of the persistent sampling kernels (csrc/generate.hip, csrc/vae_generate.hip) refuse, and what
they accept, argument by argument.

A HOST test, and only a host test: every call here passes host pointers.  A refused call returns -1 before it touches a
device; an accepted one goes on to the launch, which without a device fails with a positive HIP error and with one would run
a kernel on host addresses.  So the module skips itself wherever a GPU is visible.

Each entry point gets one acceptable call (N = T = nsteps = S = 1, D = H = 88, L = 2, C = 4, every pointer one small 16-byte
aligned buffer), then every argument but the stream is perturbed singly, then come the cases that need several arguments: the
32-bit addressing limits and the rules of single entry points.  The expected outcome of every case is the literal table
below, recorded from the library as it was before the entry points were folded onto one launcher per family: the refuse side
catches a check that got lost, the accept side one that became too strict."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib

pytestmark = pytest.mark.skipif(_lib.lib().clv_device_count() > 0, reason="host pointers: an accepted call would launch on them")

VRNN_ENC, VRNN_DEC = "Kx_enc Kw_enc b_enc U_enc Wz bz", "Kx_dec Kz Kw_dec b_dec U_dec Wo bo"
VAE_ENC, VAE_DEC = "Kh bh Kz bz", "Kd bd Ko bo"
GENERATE = {"vrnn": "N S nsteps D H L C gate_act z_prior seed x_seed w", "vae": "N nsteps D H L C use_x_prev z_prior seed x_seed w"}
FLAG = {"vrnn": "gate_act", "vae": "use_x_prev"}
TEMPER = "clamp inv_temperature z_temperature"


def _arguments():
    """entry point -> its argument names, in the order of include/clvae.h"""
    out = {}
    for fam, enc, dec in (("vrnn", VRNN_ENC, VRNN_DEC), ("vae", VAE_ENC, VAE_DEC)):
        weights, vary = enc + " " + dec, "N T D H L C %s hist_source seed sources x0 w_enc w_dec " % FLAG[fam]
        out["clv_%s_generate" % fam] = " ".join((GENERATE[fam], weights, "Xs xhat stream"))
        out["clv_%s_generate_clamped" % fam] = " ".join((GENERATE[fam], weights, "clamp Xs xhat stream"))
        out["clv_%s_generate_tempered" % fam] = " ".join((GENERATE[fam], weights, TEMPER, "Xs xhat stream"))
        out["clv_%s_vary" % fam] = " ".join((vary + weights, TEMPER, "Xs xhat stream"))
        out["clv_%s_vary_latents" % fam] = " ".join((vary + weights, TEMPER, "Xs xhat zout stream"))
        out["clv_%s_decode" % fam] = " ".join(("N T D H L C %s seed z_in x0 history w_dec noise_rows" % FLAG[fam], dec,
                                               "clamp inv_temperature Xs xhat stream"))
    return {k: v.split() for k, v in out.items()}


ARGUMENTS = _arguments()
INTS = dict(N=1, S=1, nsteps=1, T=1, D=88, H=88, L=2, C=4, gate_act=0, use_x_prev=1, z_prior=0, hist_source=0)
FLOATS = ("inv_temperature", "z_temperature")
INT_VALUES = (0, -1, 2, 33, 87, 2 ** 20, 1)
SEED_VALUES = (0, 2, 33, 87, 2 ** 20, 2 ** 64 - 1)
FLOAT_VALUES = (0.0, -1.0, float("nan"), float("inf"))

_buffer = np.zeros(64, np.float32)
BUF = _buffer.ctypes.data + (-_buffer.ctypes.data) % 16          # 16-byte aligned, 32 floats behind it


def acceptable(name):
    return {a: INTS[a] if a in INTS else 1 if a == "seed" else 1.0 if a in FLOATS else None if a == "stream" else BUF
            for a in ARGUMENTS[name]}


def perturbations(arg):
    """the values an argument takes in turn; EXPECTED holds one letter for each, in this order"""
    if arg in INTS:
        return INT_VALUES
    if arg == "seed":
        return SEED_VALUES
    return FLOAT_VALUES if arg in FLOATS else (None, BUF + 4)


def outcome(name, **changed):
    """'R': refused (-1).  'A': accepted, which without a device ends in a positive HIP error."""
    args = dict(acceptable(name), **changed)
    assert set(args) == set(ARGUMENTS[name]), set(args) ^ set(ARGUMENTS[name])
    code = getattr(_lib.lib(), name)(*[args[a] for a in ARGUMENTS[name]])
    assert code == -1 or code > 0, (name, changed, code)
    return "R" if code == -1 else "A"


# entry point -> argument -> the outcomes of perturbations(argument)
EXPECTED = {
    'clv_vrnn_generate': dict(N='RRAAAAA', S='ARAAAAA', nsteps='ARAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA',
        C='RRARRRA', gate_act='ARRRRRA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kx_enc='RR', Kw_enc='RA',
        b_enc='RA', U_enc='RA', Wz='RA', bz='RA', Kx_dec='AA', Kz='RA', Kw_dec='RA', b_dec='RA', U_dec='RA', Wo='RA',
        bo='RA', Xs='RA', xhat='AA'),
    'clv_vrnn_generate_clamped': dict(N='RRAAAAA', S='ARAAAAA', nsteps='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA',
        C='RRARRRA', gate_act='ARRRRRA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kx_enc='RR', Kw_enc='RA',
        b_enc='RA', U_enc='RA', Wz='RA', bz='RA', Kx_dec='AA', Kz='RA', Kw_dec='RA', b_dec='RA', U_dec='RA', Wo='RA',
        bo='RA', clamp='RA', Xs='RA', xhat='AA'),
    'clv_vrnn_generate_tempered': dict(N='RRAAAAA', S='ARAAAAA', nsteps='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA',
        C='RRARRRA', gate_act='ARRRRRA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kx_enc='RR', Kw_enc='RA',
        b_enc='RA', U_enc='RA', Wz='RA', bz='RA', Kx_dec='AA', Kz='RA', Kw_dec='RA', b_dec='RA', U_dec='RA', Wo='RA',
        bo='RA', clamp='AA', inv_temperature='RRRR', z_temperature='ARRR', Xs='RA', xhat='AA'),
    'clv_vrnn_vary': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA', gate_act='ARRRRRA',
        hist_source='AAAAAAA', seed='AAAAAA', sources='RA', x0='AA', w_enc='RA', w_dec='RA', Kx_enc='RR', Kw_enc='RA',
        b_enc='RA', U_enc='RA', Wz='RA', bz='RA', Kx_dec='AA', Kz='RA', Kw_dec='RA', b_dec='RA', U_dec='RA', Wo='RA',
        bo='RA', clamp='AA', inv_temperature='RRRR', z_temperature='ARRR', Xs='RA', xhat='AA'),
    'clv_vrnn_vary_latents': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        gate_act='ARRRRRA', hist_source='AAAAAAA', seed='AAAAAA', sources='RA', x0='AA', w_enc='RA', w_dec='RA',
        Kx_enc='RR', Kw_enc='RA', b_enc='RA', U_enc='RA', Wz='RA', bz='RA', Kx_dec='AA', Kz='RA', Kw_dec='RA', b_dec='RA',
        U_dec='RA', Wo='RA', bo='RA', clamp='AA', inv_temperature='RRRR', z_temperature='ARRR', Xs='RA', xhat='AA',
        zout='AA'),
    'clv_vrnn_decode': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        gate_act='ARRRRRA', seed='AAAAAA', z_in='RA', x0='AA', history='AA', w_dec='RA', noise_rows='AA', Kx_dec='AA',
        Kz='RA', Kw_dec='RA', b_dec='RA', U_dec='RA', Wo='RA', bo='RA', clamp='AA', inv_temperature='RRRR', Xs='RA',
        xhat='AA'),
    'clv_vae_generate': dict(N='RRAAAAA', nsteps='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kh='RA', bh='RA', Kz='RA', bz='RA',
        Kd='RA', bd='RA', Ko='RA', bo='RA', Xs='RA', xhat='AA'),
    'clv_vae_generate_clamped': dict(N='RRAAAAA', nsteps='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kh='RA', bh='RA', Kz='RA', bz='RA',
        Kd='RA', bd='RA', Ko='RA', bo='RA', clamp='RA', Xs='RA', xhat='AA'),
    'clv_vae_generate_tempered': dict(N='RRAAAAA', nsteps='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', z_prior='AAAAAAA', seed='AAAAAA', x_seed='RA', w='RA', Kh='RA', bh='RA', Kz='RA', bz='RA',
        Kd='RA', bd='RA', Ko='RA', bo='RA', clamp='AA', inv_temperature='RRRR', z_temperature='ARRR', Xs='RA', xhat='AA'),
    'clv_vae_vary': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', hist_source='AAAAAAA', seed='AAAAAA', sources='RA', x0='AA', w_enc='RA', w_dec='RA', Kh='RA',
        bh='RA', Kz='RA', bz='RA', Kd='RA', bd='RA', Ko='RA', bo='RA', clamp='AA', inv_temperature='RRRR',
        z_temperature='ARRR', Xs='RA', xhat='AA'),
    'clv_vae_vary_latents': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', hist_source='AAAAAAA', seed='AAAAAA', sources='RA', x0='AA', w_enc='RA', w_dec='RA', Kh='RA',
        bh='RA', Kz='RA', bz='RA', Kd='RA', bd='RA', Ko='RA', bo='RA', clamp='AA', inv_temperature='RRRR',
        z_temperature='ARRR', Xs='RA', xhat='AA', zout='AA'),
    'clv_vae_decode': dict(N='RRAAAAA', T='RRAAAAA', D='RRRRRRR', H='RRRRRRR', L='RRARRRA', C='RRARRRA',
        use_x_prev='AAAAAAA', seed='AAAAAA', z_in='RA', x0='AA', history='AA', w_dec='RA', noise_rows='AA', Kd='RA',
        bd='RA', Ko='RA', bo='RA', clamp='AA', inv_temperature='RRRR', Xs='RA', xhat='AA'),
}

# (entry point, changed arguments, outcome): the cases that take more than one argument
P20, P16, P11, P10 = 2 ** 20, 2 ** 16, 2 ** 11, 2 ** 10
SEVERAL = [
    # N*T*L >= 2^32 with a zout (the roll taken away: cl_vrnn bounds N*T*88 with one)
    ("clv_vrnn_vary_latents", dict(N=P20, T=P11, clamp=None), "R"),
    ("clv_vae_vary_latents", dict(N=P20, T=P11, clamp=None), "R"),
    ("clv_vrnn_vary_latents", dict(N=P20, T=P11 - 1, clamp=None), "A"),
    ("clv_vae_vary_latents", dict(N=P20, T=P11 - 1, clamp=None), "A"),
    ("clv_vrnn_vary_latents", dict(N=P20, T=P11, clamp=None, zout=None), "A"),
    ("clv_vae_vary_latents", dict(N=P20, T=P11, clamp=None, zout=None), "A"),
    ("clv_vrnn_vary", dict(N=P20, T=P11, clamp=None), "A"),
    ("clv_vae_vary", dict(N=P20, T=P11, clamp=None), "A"),
    # N*nsteps*88 >= 2^32 with a roll: 2^16 * 745 * 88 is the first product past 2^32.  cl_vae sets no such bound
    ("clv_vrnn_generate_clamped", dict(N=P16, nsteps=745), "R"),
    ("clv_vrnn_generate_clamped", dict(N=P16, nsteps=744), "A"),
    ("clv_vrnn_generate_tempered", dict(N=P16, nsteps=745), "R"),
    ("clv_vrnn_generate_tempered", dict(N=P16, nsteps=744), "A"),
    ("clv_vrnn_generate_tempered", dict(N=P16, nsteps=745, clamp=None), "A"),
    ("clv_vrnn_generate", dict(N=P16, nsteps=745), "A"),
    ("clv_vrnn_vary", dict(N=P16, T=745), "R"),
    ("clv_vrnn_vary", dict(N=P16, T=744), "A"),
    ("clv_vrnn_vary", dict(N=P16, T=745, clamp=None), "A"),
    ("clv_vrnn_vary_latents", dict(N=P16, T=745), "R"),
    ("clv_vrnn_vary_latents", dict(N=P16, T=744), "A"),
    ("clv_vae_generate", dict(N=P16, nsteps=745), "A"),
    ("clv_vae_generate_clamped", dict(N=P16, nsteps=745), "A"),
    ("clv_vae_generate_tempered", dict(N=P16, nsteps=745), "A"),
    ("clv_vae_vary", dict(N=P16, T=745), "A"),
    ("clv_vae_vary_latents", dict(N=P16, T=745), "A"),
    # T*88*4 >= 2^32 for cl_vrnn's re-decoding: T = 12201612 is the first; cl_vae sets no such bound
    ("clv_vrnn_vary", dict(T=12201612, clamp=None), "R"),
    ("clv_vrnn_vary", dict(T=12201611, clamp=None), "A"),
    ("clv_vrnn_vary_latents", dict(T=12201612, clamp=None), "R"),
    ("clv_vrnn_vary_latents", dict(T=12201611, clamp=None), "A"),
    ("clv_vae_vary", dict(T=2 ** 24), "A"),
    ("clv_vae_vary_latents", dict(T=2 ** 24), "A"),
    # N*T*88 >= 2^32 for decoding, roll or not
    ("clv_vrnn_decode", dict(N=P16, T=745, L=1, clamp=None), "R"),
    ("clv_vrnn_decode", dict(N=P16, T=744, L=1), "A"),
    ("clv_vae_decode", dict(N=P16, T=745, L=1, clamp=None), "R"),
    ("clv_vae_decode", dict(N=P16, T=744, L=1), "A"),
    # one entry point's own: _clamped is the roll; seed frames only where S > 0
    ("clv_vrnn_generate_clamped", dict(clamp=None), "R"),
    ("clv_vae_generate_clamped", dict(clamp=None), "R"),
    ("clv_vrnn_generate", dict(S=0, x_seed=None), "A"),
    ("clv_vrnn_generate_clamped", dict(S=0, x_seed=None), "A"),
    ("clv_vrnn_generate_tempered", dict(S=0, x_seed=None), "A"),
    ("clv_vrnn_generate", dict(S=2, x_seed=None), "R"),
    # nsteps = 0 with and without Xs: cl_vrnn may run its seed frames alone, but not under a roll; cl_vae never
    ("clv_vrnn_generate", dict(nsteps=0), "A"),
    ("clv_vrnn_generate", dict(nsteps=0, Xs=None), "A"),
    ("clv_vrnn_generate", dict(nsteps=0, S=0), "R"),
    ("clv_vrnn_generate_clamped", dict(nsteps=0), "R"),
    ("clv_vrnn_generate_clamped", dict(nsteps=0, Xs=None), "R"),
    ("clv_vrnn_generate_tempered", dict(nsteps=0), "R"),
    ("clv_vrnn_generate_tempered", dict(nsteps=0, clamp=None), "A"),
    ("clv_vrnn_generate_tempered", dict(nsteps=0, clamp=None, Xs=None), "A"),
    ("clv_vae_generate", dict(nsteps=0, Xs=None), "R"),
    ("clv_vae_generate_clamped", dict(nsteps=0, Xs=None), "R"),
    ("clv_vae_generate_tempered", dict(nsteps=0, clamp=None, Xs=None), "R"),
    ("clv_vrnn_vary", dict(T=0, Xs=None), "R"),
    ("clv_vae_vary", dict(T=0, Xs=None), "R"),
    ("clv_vrnn_decode", dict(T=0, Xs=None), "R"),
    ("clv_vae_decode", dict(T=0, Xs=None), "R"),
]


def test_the_tables_cover_every_entry_point_and_argument():
    assert set(EXPECTED) == set(ARGUMENTS) and len(ARGUMENTS) == 12
    for name, args in ARGUMENTS.items():
        assert len(args) == len(_lib.SIGNATURES[name][1]), name
        assert set(EXPECTED[name]) == set(args) - {"stream"}, name
        for a in EXPECTED[name]:
            assert len(EXPECTED[name][a]) == len(perturbations(a)), (name, a)
    assert {c[0] for c in SEVERAL} == set(ARGUMENTS)


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_every_argument_perturbed_singly(name):
    assert outcome(name) == "A"
    got = {a: "".join(outcome(name, **{a: v}) for v in perturbations(a)) for a in ARGUMENTS[name] if a != "stream"}
    assert got == EXPECTED[name]


def test_cases_of_several_arguments():
    got = [(name, changed, outcome(name, **changed)) for name, changed, _ in SEVERAL]
    assert got == SEVERAL
