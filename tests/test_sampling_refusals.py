"""What the six entry points of the persistent sampling kernels (csrc/generate.hip, csrc/vae_generate.hip) refuse, and what
they accept, argument by argument, in the twelve forms of call that were entry points of their own before ABI 610.

A HOST test, and only a host test: every call here passes host pointers.  A refused call returns -1 before it touches a
device; an accepted one goes on to the launch, which without a device fails with a positive HIP error and with one would run
a kernel on host addresses.  So the module skips itself wherever a GPU is visible.

Each form gets one acceptable call (N = T = nsteps = S = 1, D = H = 88, L = 2, C = 4, every pointer one small 16-byte
aligned buffer), then every argument but the stream is perturbed singly, then come the cases that need several arguments: the
32-bit addressing limits and the rules of single entry points.  The expected outcome of every case is the literal table
below, recorded from the library as it was before the entry points were folded onto one launcher per family and keyed by the
twelve names of that library: the refuse side catches a check that got lost, the accept side one that became too strict.
outcome() translates a form to its folded entry point (FOLDED: plain is clamp = NULL, tempered = 0, both factors 1, t0 = 0, no
states; _clamped is tempered = 0; _tempered is tempered = 1; _vary is zout = NULL), so the table proves that the fold lost and
gained no refusal.  Exactly four cells differ from the record, because their refusal belonged to a symbol that is gone:
_generate_clamped refused a NULL roll, which is now the plain call -- clamp = 'RA' became 'AA' in the two _clamped rows of
EXPECTED, and the two SEVERAL cases (clv_*_generate_clamped, clamp=None) became 'A'.  What the fold added (tempered, t0, the
two states, and the rules between them) has tables of its own, NEW and the end of SEVERAL, recorded from the folded library."""
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
GENERATE_TAIL = "clamp tempered inv_temperature z_temperature t0 state_in state_out Xs xhat stream".split()
# the six entry points of include/clvae.h -> their argument names, in its order
REAL = {"clv_%s_%s" % (fam, op): args for fam in ("vrnn", "vae") for op, args in (
    ("generate", ARGUMENTS["clv_%s_generate" % fam][:-3] + GENERATE_TAIL),
    ("vary", ARGUMENTS["clv_%s_vary_latents" % fam]), ("decode", ARGUMENTS["clv_%s_decode" % fam]))}
UNTEMPERED, NO_STATE = dict(tempered=0, inv_temperature=1.0, z_temperature=1.0), dict(t0=0, state_in=None, state_out=None)
# (a form's suffix, the suffix of the entry point that took it over, the arguments of that entry point the form does not have)
FORMS = (("_generate", "_generate", dict(clamp=None, **UNTEMPERED, **NO_STATE)),
         ("_generate_clamped", "_generate", dict(UNTEMPERED, **NO_STATE)),
         ("_generate_tempered", "_generate", dict(tempered=1, **NO_STATE)),
         ("_vary", "_vary", dict(zout=None)), ("_vary_latents", "_vary", {}), ("_decode", "_decode", {}))
FOLDED = {"clv_" + fam + form: ("clv_" + fam + real, fill) for fam in ("vrnn", "vae") for form, real, fill in FORMS}
INTS = dict(N=1, S=1, nsteps=1, T=1, D=88, H=88, L=2, C=4, gate_act=0, use_x_prev=1, z_prior=0, hist_source=0, tempered=0)
FLOATS = ("inv_temperature", "z_temperature")
INT_VALUES = (0, -1, 2, 33, 87, 2 ** 20, 1)
SEED_VALUES = (0, 2, 33, 87, 2 ** 20, 2 ** 64 - 1)
T0_VALUES = (0, 2, 33, 87, 2 ** 20, 2 ** 32 - 1)
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
    if arg == "t0":
        return T0_VALUES
    return FLOAT_VALUES if arg in FLOATS else (None, BUF + 4)


def outcome(name, **changed):
    """'R': refused (-1).  'A': accepted, which without a device ends in a positive HIP error.  name: one of the twelve
    forms; changed: arguments of the form, or of the entry point that took it over"""
    real, fill = FOLDED[name]
    args = dict(fill, **dict(acceptable(name), **changed))
    assert set(args) == set(REAL[real]), set(args) ^ set(REAL[real])
    code = getattr(_lib.lib(), real)(*[args[a] for a in REAL[real]])
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
        bo='RA', clamp='AA', Xs='RA', xhat='AA'),
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
        Kd='RA', bd='RA', Ko='RA', bo='RA', clamp='AA', Xs='RA', xhat='AA'),
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
    # one entry point's own: a _clamped call without its roll is the plain call (before 610: refused); seed frames only
    # where S > 0
    ("clv_vrnn_generate_clamped", dict(clamp=None), "A"),
    ("clv_vae_generate_clamped", dict(clamp=None), "A"),
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
    # ---- new with the fold (the plain form, S = nsteps = 1, with the arguments that 610 added)
    # tempered = 0 is the untempered call: both factors must be 1; tempered = 1 takes any factor the tempered model allows
    ("clv_vrnn_generate", dict(inv_temperature=0.5), "R"),
    ("clv_vrnn_generate", dict(z_temperature=0.5), "R"),
    ("clv_vrnn_generate", dict(tempered=1, inv_temperature=0.5, z_temperature=0.0), "A"),
    ("clv_vrnn_generate", dict(tempered=1, inv_temperature=0.0), "R"),
    ("clv_vae_generate", dict(inv_temperature=0.5), "R"),
    ("clv_vae_generate", dict(z_temperature=0.5), "R"),
    ("clv_vae_generate", dict(tempered=1, inv_temperature=0.5, z_temperature=0.0), "A"),
    ("clv_vae_generate", dict(tempered=1, inv_temperature=0.0), "R"),
    # ... from and to a state too, where the flag picks no kernel
    ("clv_vrnn_generate", dict(t0=1, inv_temperature=0.5), "R"),
    ("clv_vrnn_generate", dict(t0=1, tempered=1, inv_temperature=0.5), "A"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, z_temperature=0.5), "R"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, tempered=1, z_temperature=0.5), "A"),
    # cl_vrnn from / to a state: state_in NULL is the zero start; the seed and Xs only where S > 0 / nsteps > 0; a roll
    # needs a returned frame; t0 + S + nsteps <= 2^32 - 1
    ("clv_vrnn_generate", dict(state_in=BUF, state_out=BUF, t0=5, clamp=BUF), "A"),
    ("clv_vrnn_generate", dict(state_in=BUF, S=0, x_seed=None), "A"),
    ("clv_vrnn_generate", dict(state_in=BUF, S=2, x_seed=None), "R"),
    ("clv_vrnn_generate", dict(state_out=BUF, nsteps=0, Xs=None), "A"),
    ("clv_vrnn_generate", dict(state_out=BUF, nsteps=0, clamp=BUF), "R"),
    ("clv_vrnn_generate", dict(state_in=BUF, S=0, nsteps=0), "R"),
    ("clv_vrnn_generate", dict(t0=2 ** 32 - 3), "A"),
    ("clv_vrnn_generate", dict(t0=2 ** 32 - 2), "R"),
    ("clv_vrnn_generate", dict(t0=2 ** 32 - 2, state_in=BUF, state_out=BUF), "R"),
    ("clv_vrnn_generate", dict(t0=2 ** 31, S=2 ** 30, nsteps=2 ** 30 - 1, state_in=BUF), "A"),
    ("clv_vrnn_generate", dict(t0=2 ** 31, S=2 ** 30, nsteps=2 ** 30, state_in=BUF), "R"),
    # cl_vae from / to a state: the state stands for the seed frame -- state_in is required, x_seed must be NULL;
    # t0 + nsteps <= 2^32 - 1
    ("clv_vae_generate", dict(state_in=BUF), "R"),
    ("clv_vae_generate", dict(state_in=BUF, state_out=BUF, t0=5), "R"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF), "A"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, state_out=BUF, t0=5, clamp=BUF), "A"),
    ("clv_vae_generate", dict(x_seed=None, state_out=BUF), "R"),
    ("clv_vae_generate", dict(x_seed=None, t0=1), "R"),
    ("clv_vae_generate", dict(x_seed=None), "R"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, t0=2 ** 32 - 2), "A"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, t0=2 ** 32 - 1), "R"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, t0=2 ** 31, nsteps=2 ** 31 - 1), "A"),
    ("clv_vae_generate", dict(x_seed=None, state_in=BUF, t0=2 ** 31, nsteps=2 ** 31), "R"),
]

# the arguments that the fold added to the two generate entry points, perturbed singly from the plain form (which gives its
# seed frame: in cl_vae anything that makes the call one from / to a state then contradicts it) and, cl_vae, from the form
# from a state (x_seed NULL, state_in given)
NEW = {
    'clv_vrnn_generate': ({}, dict(tempered='AAAAAAA', t0='AAAAAR', state_in='AA', state_out='AA')),
    'clv_vae_generate': ({}, dict(tempered='AAAAAAA', t0='ARRRRR', state_in='AR', state_out='AR')),
    'clv_vae_generate from a state': (dict(x_seed=None, state_in=BUF), dict(tempered='AAAAAAA', t0='AAAAAR', state_in='RA',
                                                                           state_out='AA')),
}


def test_the_tables_cover_every_entry_point_and_argument():
    assert set(EXPECTED) == set(ARGUMENTS) == set(FOLDED) and len(ARGUMENTS) == 12
    assert len(REAL) == 6 and {real for real, _ in FOLDED.values()} == set(REAL)
    for name, args in REAL.items():
        assert len(args) == len(set(args)) == len(_lib.SIGNATURES[name][1]), name
    assert [len(REAL["clv_%s_%s" % (fam, op)]) for op in ("generate", "vary", "decode") for fam in ("vrnn", "vae")] \
        == [35, 29, 33, 28, 25, 22]
    for name in set(ARGUMENTS) - set(REAL):                  # the six names that 610 removed
        assert name not in _lib.SIGNATURES and not hasattr(_lib.lib(), name), name
    for name, args in ARGUMENTS.items():
        real, fill = FOLDED[name]
        assert set(args) | set(fill) == set(REAL[real]) and not set(args) & set(fill), name      # a form + its fill = one call
        assert [a for a in REAL[real] if a in args] == args, name                                # in the entry point's order
        assert set(EXPECTED[name]) == set(args) - {"stream"}, name
        for a in EXPECTED[name]:
            assert len(EXPECTED[name][a]) == len(perturbations(a)), (name, a)
    assert {c[0] for c in SEVERAL} == set(ARGUMENTS)
    for name, (base, table) in NEW.items():
        assert set(table) == set(GENERATE_TAIL) - set(ARGUMENTS[name.split()[0] + "_tempered"]), name
        for a in table:
            assert len(table[a]) == len(perturbations(a)), (name, a)


@pytest.mark.parametrize("name", sorted(ARGUMENTS))
def test_every_argument_perturbed_singly(name):
    assert outcome(name) == "A"
    got = {a: "".join(outcome(name, **{a: v}) for v in perturbations(a)) for a in ARGUMENTS[name] if a != "stream"}
    assert got == EXPECTED[name]


@pytest.mark.parametrize("name", sorted(NEW))
def test_every_new_argument_perturbed_singly(name):
    base, table = NEW[name]
    form = name.split()[0]
    assert outcome(form, **base) == "A"
    got = {a: "".join(outcome(form, **dict(base, **{a: v})) for v in perturbations(a)) for a in table}
    assert got == table


def test_cases_of_several_arguments():
    got = [(name, changed, outcome(name, **changed)) for name, changed, _ in SEVERAL]
    assert got == SEVERAL
