"""The pair kernels' chains (csrc/lstm_pair.hip) keep two record sets in flight, requested two steps ahead; that holds only
while every wait of a step loop is a counted one that leaves the other set's loads outstanding.  A wait for everything can
come from register allocation alone -- a packed operand with an undefined half beside a register a load is writing
(DESIGN.md 8 item 6 iii) -- so only the compiled loops show it.  Likewise the hW rescale's walk over the partial rows
(csrc/optim.hip) must not fall back to one load per wait.  tools/pair_waits.py reads the assembly; two compiles side by
side (about a minute), no GPU.

The table asserted below is today's, per instance and loop in program order:
  forward <G, X, Z, XL = 0>   chains [4, 4], latent wave [9, 8, 9, 8]
  forward <G, X, Z, XL = 1>   chains [13, 12, 13, 12], latent wave [18, 16, 18, 16] (the frame rows are gathered in the kernel:
                              eight row loads and the next note list per step; the 9th.. note path is a nested loop that
                              waits for one load at a time on purpose and is printed apart)
  backward <G, ZP, WZG = 1>   encoder chain [5, 5], latent wave [12, 10, 9, 12, 10, 9], decoder chain [5, 5]
  backward <G, ZP, WZG = 0>   encoder chain [4, 4], the rest as above
A forward instance without a decoder projection (X = 0) lists two loops instead of three: one chain's loop then has fewer
than two vector loads per iteration and is no step loop by the tool's definition.
Before the pin in matvec, backward <G, 4, 1>'s encoder chain read [5, 0]."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOP = re.compile(r"^(lstm_pair_(fwd|bwd)_kernel<([\d,]+)>): step loop \S+ (\d) steps: (\d+) loads, (\d+) stores, vmcnt \[([\d, ]*)\]$")


@pytest.fixture(scope="module")
def report():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the assembly cannot be produced")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pair_waits.py")], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def table(lines):
    """{instance: [vmcnt list of each step loop, in program order]}"""
    out = {}
    for l in lines:
        m = LOOP.match(l)
        if m:
            assert m.group(4) == "2", l                     # every step loop is a two-step loop
            out.setdefault(m.group(1), []).append([int(x) for x in m.group(7).split(",") if x.strip()])
    return out


def test_instances_and_rules(report):
    assert report[-1] == "16 forward and 12 backward instances, 1 rescale kernel, 0 fail", report[-1]
    assert not any("FAIL" in l for l in report)
    t = table(report)
    assert sum(k.startswith("lstm_pair_fwd") for k in t) == 16           # G 2 x X 2 x Z 2 x XL 2
    assert sum(k.startswith("lstm_pair_bwd") for k in t) == 12           # G 2 x ZP 3 x WZG 2


def test_wait_table(report):
    t = table(report)
    for g in (0, 1):
        for x in (0, 1):
            for z in (1, 2):
                for xl in (0, 1):
                    chain, latw = ([13, 12, 13, 12], [18, 16, 18, 16]) if xl else ([4, 4], [9, 8, 9, 8])
                    want = [chain, latw, chain] if x else [latw, chain]
                    assert t["lstm_pair_fwd_kernel<%d,%d,%d,%d>" % (g, x, z, xl)] == want, (g, x, z, xl)
        for zp in (4, 8, 16):
            for wzg in (0, 1):
                want = [[5, 5] if wzg else [4, 4], [12, 10, 9, 12, 10, 9], [5, 5]]
                assert t["lstm_pair_bwd_kernel<%d,%d,%d>" % (g, zp, wzg)] == want, (g, zp, wzg)


def test_rescale_walk_requests_its_rows_together(report):
    walk = [l for l in report if l.startswith("wn_fast_rescale_kernel: walk loop")]
    assert len(walk) == 1, walk
    m = re.search(r": (\d+) loads, vmcnt \[([\d, ]*)\]$", walk[0])
    waits = [int(x) for x in m.group(2).split(",")]
    assert int(m.group(1)) == 12 and waits == list(range(11, -1, -1)), walk[0]      # one round: 12 loads, then counted waits
