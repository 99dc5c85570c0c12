"""The producers of csrc/wgrad_bf16.hip keep two stages of operand loads in flight only while the compiler can count the
loads between a request and its use; a compiler update (or an edit that puts a load behind a condition) silently turns
the counted waits into vmcnt(0) and costs a memory latency per stage.  tools/wgrad_waits.py reads the compiled loop; one
compile of the file (about 20 s), no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_producer_loops_wait_with_counted_vmcnt():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the assembly cannot be produced")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "wgrad_waits.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("12 instances, 0 fail"), lines[-1]        # HM 6 / 8 x (XP 1 u8, XP 1, XP 3) x (single, pair)
    assert not any("vmcnt 0 " in l or l.endswith(" 0") for l in lines if l.startswith("  half"))
