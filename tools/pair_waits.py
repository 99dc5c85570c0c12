"""What the step loops of the pair kernels (csrc/lstm_pair.hip) and the partial-row walk of the hW rescale (csrc/optim.hip,
wn_fast_rescale_kernel) wait for: compiles both files to gfx950 assembly with the Makefile's own lines and prints, for every
lstm_pair_fwd_kernel / lstm_pair_bwd_kernel instance, each step loop -- a loop with a barrier and at least two vector
loads -- as the sequence of its vector loads, stores, barriers and `s_waitcnt vmcnt(n)`, in program order.

The chains keep two record sets in flight (rA, rB: requested two steps ahead, the loop body is two steps), the latent waves
likewise.  That only works while every wait between a request and its use is a COUNTED one that leaves the other set in
flight.  A wait for everything can come from the source (a load behind a condition) or from register allocation alone: a
packed operand whose unused half lands beside a register a load is writing (DESIGN.md 8 item 6 iii).  Only the assembly
shows the second kind.  Exit status 1 if
  * a step loop holds a `vmcnt(0)`,
  * a half of a two-step loop has no `vmcnt` wait,
  * the first wait of a half is below the number of vector memory operations (loads plus stores) of the other half, or
  * a loop of the rescale kernel issues one load per `vmcnt(0)` (a load-wait-add walk: one memory latency per row).
  python tools/pair_waits.py [--asm-pair FILE.s] [--asm-optim FILE.s] [--keep DIR]"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc")
FWD = re.compile(r"^_ZN3clv\d+(lstm_pair_fwd_kernel)ILi(\d+)ELb(\d)ELi(\d+)ELb(\d)EEEv\w+:")
BWD = re.compile(r"^_ZN3clv\d+(lstm_pair_bwd_kernel)ILi(\d+)ELi(\d+)ELb(\d)EEEv\w+:")
RESCALE = re.compile(r"^_ZN3clv\d+(wn_fast_rescale_kernel)E\w+:")
BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)")
HEADER = re.compile(r"Loop Header: Depth=1")
INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=1")
LOAD = re.compile(r"^\s+(?:global|buffer|flat)_load_\w+\s")
STORE = re.compile(r"^\s+(?:global|buffer|flat)_store_\w+\s")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def compile_asm(name, out):
    """The Makefile's compile line of <name>.o, turned into a device-only -S."""
    line = [l for l in subprocess.check_output(["make", "-C", CSRC, "-n", "-B", name + ".o"], text=True).splitlines()
            if name + ".hip" in l and " -c " in l]
    if not line:
        raise SystemExit("no compile line for %s.o in the Makefile" % name)
    cmd = shlex.split(line[0])
    cmd[cmd.index("-o") + 1] = out
    cmd[cmd.index("-c")] = "-S"
    cmd.insert(1, "--cuda-device-only")
    subprocess.check_call(cmd, cwd=CSRC, stderr=subprocess.DEVNULL)


def instances(text, patterns):
    """[(name, lines)] of every kernel one of the patterns matches."""
    out, cur = [], None
    for l in text.splitlines():
        m = next((m for m in (p.match(l) for p in patterns) if m), None)
        if m:
            cur = ("%s<%s>" % (m.group(1), ",".join(m.groups()[1:])) if len(m.groups()) > 1 else m.group(1), [])
            out.append(cur)
        elif cur is not None:
            if l.startswith(".Lfunc_end"):
                cur = None
            else:
                cur[1].append(l)
    return out


def loops(lines, children=None):
    """{header label: [instruction lines]} of the depth-1 loops of a function, blocks in layout order.  The blocks of a loop
    nested in one (depth 2) are left out of it and collected in children[outer header] instead: in the forward kernels
    that gather their frame rows that is the path of a frame's 9th.. note, a rare uniform branch that waits for one load
    at a time on purpose (XProj::extra) and is no part of the step's steady state."""
    body, nested, at, child = {}, {}, None, False
    for l in lines:
        m = BLOCK.match(l)
        if m:
            if HEADER.search(l) and m.group(1):
                at, child = m.group(1)[2:], False
            else:
                p, q = PARENT.search(l), INLOOP.search(l)
                if p:
                    at, child = p.group(1), True
                    nested[m.group(1)[2:]] = at
                elif q and q.group(2) == "1":
                    at, child = q.group(1), False
                elif q:
                    at, child = nested.get(q.group(1)), True
                else:
                    at = None
            if at is not None:
                body.setdefault(at, [])
        elif at is not None and l.startswith("\t"):
            if not child:
                body[at].append(l)
            elif children is not None:
                children.setdefault(at, []).append(l)
    return body


def events(loop):
    ev = []
    for l in loop:
        if LOAD.match(l):
            ev.append(("L", None))
        elif STORE.match(l):
            ev.append(("S", None))
        elif re.match(r"^\s+s_barrier\b", l):
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
    """The loop's events as one list per barrier, rotated so that each list ends with its barrier (the layout order of a
    rotated loop is a rotation of its execution order)."""
    last = max(i for i, (k, _) in enumerate(ev) if k == "B")
    ev = ev[last + 1:] + ev[:last + 1]
    out, cur = [], []
    for e in ev:
        cur.append(e)
        if e[0] == "B":
            out.append(cur)
            cur = []
    return out


def show(h):
    """program order: waits as numbers, runs of loads / stores as "[n loads]" """
    seq, run, kind = [], 0, None
    for k, n in list(h) + [(None, None)]:          # the sentinel flushes the last run
        if k in ("L", "S") and k == kind:
            run += 1
            continue
        if run:
            seq.append("[%d %s%s]" % (run, "load" if kind == "L" else "store", "s" if run > 1 else ""))
        run, kind = (1, k) if k in ("L", "S") else (0, None)
        if k == "B":
            seq.append("barrier")
        elif k == "W":
            seq.append(str(n))
    return " ".join(seq)


def check_pair(name, lines):
    children = {}
    step = [(h, events(b)) for h, b in loops(lines, children).items()]
    step = [(h, ev) for h, ev in step if sum(k == "L" for k, _ in ev) >= 2 and any(k == "B" for k, _ in ev)]
    if not step:
        print("%s: no step loop (a loop with a barrier and at least two vector loads)" % name)
        return False
    ok = True
    for head, ev in step:
        hs = halves(ev)
        nops = [sum(k in ("L", "S") for k, _ in h) for h in hs]
        print("%s: step loop .L%s, %d steps: %d loads, %d stores, vmcnt %s" % (
            name, head, len(hs), sum(k == "L" for k, _ in ev), sum(k == "S" for k, _ in ev),
            [n for h in hs for k, n in h if k == "W"]))
        if head in children:          # not held to the rules: see loops()
            print("  nested loop(s), outside the steady state: %s" % show(events(children[head])))
        for i, h in enumerate(hs):
            print("  step %d: %s" % (i + 1, show(h)))
            waits = [n for k, n in h if k == "W"]
            why = []
            if 0 in waits:
                why.append("vmcnt(0) inside the step loop")
            if len(hs) == 2:
                other = nops[i - 1]
                if not waits:
                    why.append("a step without a vmcnt wait")
                elif waits[0] < other:
                    why.append("first wait vmcnt(%d) is below the other step's %d loads and stores" % (waits[0], other))
            for w in why:
                print("    FAIL: " + w)
            ok = ok and not why
    return ok


def check_rescale(name, lines):
    """the loops of the rescale kernel that load: the walk over the partial rows"""
    walk = [(h, events(b)) for h, b in loops(lines).items()]
    walk = [(h, ev) for h, ev in walk if any(k == "L" for k, _ in ev)]
    if not walk:
        print("%s: no loop with a vector load (the partial-row walk)" % name)
        return False
    ok = True
    for head, ev in walk:
        nload, drains = sum(k == "L" for k, _ in ev), sum(1 for k, n in ev if k == "W" and n == 0)
        print("%s: walk loop .L%s: %d loads, vmcnt %s" % (name, head, nload, [n for k, n in ev if k == "W"]))
        print("  %s" % show(ev))
        if drains and nload <= drains:
            print("    FAIL: %d load(s) per %d vmcnt(0): one memory latency per row" % (nload, drains))
            ok = False
    return ok


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm-pair", help="read this assembly of lstm_pair.hip instead of compiling")
    ap.add_argument("--asm-optim", help="read this assembly of optim.hip instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly in this directory")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        d = a.keep or d
        os.makedirs(d, exist_ok=True)
        paths = {"lstm_pair": a.asm_pair, "optim": a.asm_optim}
        todo = [n for n, p in paths.items() if not p]
        for n in todo:
            paths[n] = os.path.abspath(os.path.join(d, n + ".s"))
        with ThreadPoolExecutor(2) as ex:          # the two compiles side by side
            list(ex.map(lambda n: compile_asm(n, paths[n]), todo))
        text = {n: open(p).read() for n, p in paths.items()}
    pair = instances(text["lstm_pair"], (FWD, BWD))
    resc = instances(text["optim"], (RESCALE,))
    if not pair:
        raise SystemExit("no lstm_pair kernel in the assembly")
    if not resc:
        raise SystemExit("no wn_fast_rescale_kernel in the assembly")
    bad = [n for n, l in pair if not check_pair(n, l)] + [n for n, l in resc if not check_rescale(n, l)]
    nf = sum(n.startswith("lstm_pair_fwd") for n, _ in pair)
    print("%d forward and %d backward instances, %d rescale kernel, %d fail%s" % (nf, len(pair) - nf, len(resc), len(bad),
                                                                              (": " + ", ".join(bad)) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
