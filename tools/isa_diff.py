"""Compare the gfx950 ISA of two device-assembly dumps kernel by kernel (hipcc -S
--cuda-device-only): prints, per kernel symbol, whether its instruction stream is identical once
labels and comments are normalised.  Used to show that a source refactor leaves the shipped
kernels' code unchanged (same instructions => same bits, same time).  For a kernel that differs
it also prints the registers, scratch and LDS the two dumps' metadata state, and whether the two
streams hold the same opcodes the same number of times (a reordering)."""
import collections
import re
import sys

RESOURCES = ('vgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')


def kernels(path):
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r'^(_Z\S+):\s*(;.*)?$', line)
        if m:
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith('.Lfunc_end'):
            out[name] = cur
            name = None
            continue
        s = line.split(';')[0].strip()
        if not s or s.startswith('.'):
            continue
        s = re.sub(r'\.LBB\d+_\d+', 'L', s)
        cur.append(s)
    return out


def resources(path):
    """{kernel symbol: {field: value}} from the amdhsa.kernels metadata (fields sorted by name)."""
    out, cur = {}, {}
    for line in open(path):
        if line.startswith('  - .'):  # the next kernel's entry
            cur = {}
        m = re.match(r'^\s+(?:- )?\.(\w+):\s+(\S+)\s*$', line)
        if not m:
            continue
        if m.group(1) == 'name' and m.group(2).startswith('_Z'):
            out[m.group(2)] = cur
        elif m.group(1) in RESOURCES:
            cur[m.group(1)] = int(m.group(2))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    ra, rb = resources(sys.argv[1]), resources(sys.argv[2])
    for n in sorted(set(a) | set(b)):
        if n not in a or n not in b:
            print(f"{'only-before' if n in a else 'only-after ':11s} {n}")
            continue
        same = a[n] == b[n]
        print(f"{'same' if same else 'DIFF':11s} {n} ({len(a[n])} -> {len(b[n])} instrs)")
        if not same:
            ops = [collections.Counter(s.split()[0] for s in k[n]) for k in (a, b)]
            res = ', '.join(f"{f} {ra[n].get(f)} -> {rb[n].get(f)}" for f in RESOURCES)
            print(f"{'':11s} {res}; opcode multiset {'equal' if ops[0] == ops[1] else 'differs'}")


if __name__ == '__main__':
    main()
