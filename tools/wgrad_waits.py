"""What the producers of the split-bf16 kernel-gradient product (csrc/wgrad_bf16.hip) wait for: compiles the file to gfx950
assembly with the Makefile's own flags and prints, for every kernel instance, the steady-state producer loop as the sequence
of its `s_waitcnt vmcnt(n)`, its global / buffer loads and its stage barriers, in program order.

The loop keeps two stages of operand loads in flight (register sets A and B): each half converts one set and requests it
again.  That only works while the compiler can COUNT the loads between a request and its use; where it cannot (a load
behind a condition, two load sequences) it waits for everything.  Exit status 1 if, in any instance,
  * the loop holds a `vmcnt(0)`, or
  * the first wait of a half is below the number of loads of the other half (the other set's loads must stay in flight).
  python tools/wgrad_waits.py [--asm FILE.s] [--keep FILE.s]"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc")
KERNEL = re.compile(r"^(_ZN3clv(\d+)(lstm_wgrad_bf16(?:_pair)?_kernel)ILi(\d+)ELi(\d+)ELb(\d)EEEv\w+):")
BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)")
HEADER = re.compile(r"Loop Header: Depth=1")
INLOOP = re.compile(r"(?:in Loop: Header=|Parent Loop )(BB\d+_\d+)")
LOAD = re.compile(r"^\s+(?:global|buffer|flat)_load_\w+\s")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def compile_asm(out):
    """The Makefile's compile line of wgrad_bf16.o, turned into a device-only -S."""
    line = [l for l in subprocess.check_output(["make", "-C", CSRC, "-n", "-B", "wgrad_bf16.o"], text=True).splitlines()
            if "wgrad_bf16.hip" in l and " -c " in l]
    if not line:
        raise SystemExit("no compile line for wgrad_bf16.o in the Makefile")
    cmd = shlex.split(line[0])
    i = cmd.index("-o")
    cmd[i + 1] = out
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--cuda-device-only")
    subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)


def instances(text):
    """[(name, lines)] of every wgrad kernel in the assembly."""
    out, cur = [], None
    for l in text.splitlines():
        m = KERNEL.match(l)
        if m:
            cur = ("%s<%s,%s,%s>" % (m.group(3), m.group(4), m.group(5), "u8" if m.group(6) == "1" else "f32"), [])
            out.append(cur)
        elif cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
            else:
                cur[1].append(l)
    return out


def loops(lines):
    """{header label: [instruction lines]} of the depth-1 loops of a function (inner loops count into their parent)."""
    body, at = {}, None
    for l in lines:
        if BLOCK.match(l):
            m = BLOCK.match(l)
            if HEADER.search(l) and m.group(1):
                at = m.group(1)[2:]
            else:
                p = INLOOP.search(l)
                at = p.group(1) if p else None
            if at is not None:
                body.setdefault(at, [])
        elif at is not None and l.startswith("\t"):
            body[at].append(l)
    return body


def events(loop):
    ev = []
    for l in loop:
        if LOAD.match(l):
            ev.append(("L", None))
        elif "s_barrier" in l:
            ev.append(("B", None))
        else:
            w = WAIT.match(l)
            if w:
                v = VMCNT.search(w.group(1))
                if v:
                    ev.append(("W", int(v.group(1))))
                elif re.match(r"(0x)?[0-9a-f]+\b", w.group(1)):      # a raw immediate: every counter
                    ev.append(("W", 0))
    return ev


def halves(ev):
    """The loop's events as one list per stage barrier, rotated so that each list ends with its barrier."""
    if not any(k == "B" for k, _ in ev):
        return [ev]
    last = max(i for i, (k, _) in enumerate(ev) if k == "B")
    ev = ev[last + 1:] + ev[:last + 1]
    out, cur = [], []
    for e in ev:
        cur.append(e)
        if e[0] == "B":
            out.append(cur)
            cur = []
    return out


def check(name, lines):
    prod = [(h, b) for h, b in loops(lines).items() if any(LOAD.match(l) for l in b) and any("s_barrier" in l for l in b)]
    if len(prod) != 1:
        print("%s: %d loops with loads and a barrier (expected the producer loop alone)" % (name, len(prod)))
        return False
    head, body = prod[0]
    hs = halves(events(body))
    nload = [sum(1 for k, _ in h if k == "L") for h in hs]
    print("%s: producer loop .L%s, %d loads, %d stage barriers" % (name, head, sum(nload), len(hs)))
    ok = True
    for i, h in enumerate(hs):
        waits = [n for k, n in h if k == "W"]
        seq, run = [], 0
        for k, n in h:                      # program order: waits as numbers, runs of loads as "[n loads]"
            if k == "L":
                run += 1
                continue
            if run:
                seq.append("[%d loads]" % run)
                run = 0
            seq.append("barrier" if k == "B" else str(n))
        if run:
            seq.append("[%d loads]" % run)
        print("  half %d: vmcnt %s" % (i + 1, " ".join(seq)))
        other = nload[i - 1] if len(hs) > 1 else 0
        why = []
        if 0 in waits:
            why.append("vmcnt(0) inside the loop")
        if waits and waits[0] < other:
            why.append("first wait vmcnt(%d) is below the other set's %d loads" % (waits[0], other))
        if any(b > a for a, b in zip(waits, waits[1:])):
            print("    note: the waits do not step down in program order (blocks of alternative paths follow each other)")
        if not waits:
            why.append("no wait at all")
        for w in why:
            print("    FAIL: " + w)
        ok = ok and not why
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly here")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = a.keep or os.path.join(d, "wgrad_bf16.s")
            compile_asm(os.path.abspath(out))
            text = open(out).read()
    inst = instances(text)
    if not inst:
        raise SystemExit("no lstm_wgrad_bf16 kernel in the assembly")
    bad = [n for n, l in inst if not check(n, l)]
    print("%d instances, %d fail%s" % (len(inst), len(bad), (": " + ", ".join(bad)) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
