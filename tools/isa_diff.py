"""Compare the instruction streams of template instances between two builds of one HIP source (no GPU needed).
Usage: python tools/isa_diff.py OLD.s NEW.s 'old-name-regex' 'new-name-regex'
OLD.s / NEW.s: the ISA tools/kres.py leaves behind.  Kernels are paired in file order among those whose demangled names match
the two expressions; per pair the instructions (labels, directives and comments dropped, the kernel's own mangled name
and the function number in its branch labels masked) are compared one by one."""
import re
import subprocess
import sys


def kernels(path, pattern):
    text = open(path).read()
    out = []
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', text, re.S | re.M):
        name = m.group(1)
        if name.endswith('.kd'):
            continue
        dem = subprocess.run(['c++filt', name], capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout.strip()
        if not re.search(pattern, dem):
            continue
        ins = []
        for line in m.group(2).splitlines():
            line = line.split(';')[0].strip().replace(name, 'KERNEL')
            if not line or line.startswith('.') or line.endswith(':'):
                continue
            ins.append(re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\s+', ' ', line)))
        out.append((dem.split('(')[0], ins))
    return out


old, new = kernels(sys.argv[1], sys.argv[3]), kernels(sys.argv[2], sys.argv[4])
assert old and len(old) == len(new), (len(old), len(new))
bad = 0
for (no, io), (nn, inn) in zip(old, new):
    diff = [i for i, (a, b) in enumerate(zip(io, inn)) if a != b]
    same = len(io) == len(inn) and not diff
    bad += not same
    print("%-60s %-66s %6d %6d  %s" % (no, nn, len(io), len(inn), "identical" if same else "DIFFERENT at %s" % diff[:5]))
    for i in diff[:5]:
        print("    ", io[i], " | ", inn[i])
sys.exit(1 if bad else 0)
