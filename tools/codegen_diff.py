"""Per-kernel comparison of two gfx950 assembly files of one .hip source (the method of profiles/r24 / r25 *_codegen.txt):
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -Iic3net_amd/csrc --cuda-device-only -S <file> -o <out>.s
on the parent commit and on the tree, then
    python tools/codegen_diff.py parent.s tree.s
Every instruction line between a kernel's label and the end of the function is compared, comments and assembler directives dropped,
basic-block labels named by their order within the function.  A kernel the parent does not have is listed as NEW with its registers,
scratch bytes per lane (private_segment_fixed_size), static LDS and spill counts from the kernel's metadata."""
import re
import subprocess
import sys

KEYS = ['.agpr_count', '.vgpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size',
        '.group_segment_fixed_size']


def kernels(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', s, re.S | re.M):
        lines = []
        for ln in m.group(2).split('\n'):
            t = ln.split(';')[0].strip()
            if t and not (t.startswith('.') and not t.endswith(':')):
                lines.append(t)
        labels = {}
        for t in lines:
            if t.endswith(':'):
                labels.setdefault(t[:-1], 'L%d' % len(labels))
        out[m.group(1)] = [re.sub(r'\.LBB\d+_\d+', lambda mm: labels.get(mm.group(0), mm.group(0)), t) for t in lines]
    meta = {}
    for blk in re.finditer(r'- \.agpr_count:.*?\.wavefront_size:\s+\d+', s, re.S):
        b = blk.group(0)
        g = lambda k: re.search(re.escape(k) + r':\s+(\S+)', b).group(1)
        meta[g('.name')] = {k: g(k) for k in KEYS}
    return out, meta


def demangle(name):
    r = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
    return r.split('(')[0].replace('void ', '')


def main():
    parent, _ = kernels(sys.argv[1])
    tree, meta = kernels(sys.argv[2])
    print("# %-62s %13s %11s  result" % ("kernel", "parent instr.", "tree instr."))
    for n in sorted((n for n in tree if n in meta), key=demangle):
        if n in parent:
            print("%-64s %13d %11d  %s" % (demangle(n), len(parent[n]), len(tree[n]), 'IDENTICAL' if parent[n] == tree[n] else 'DIFFERENT'))
        else:
            m = meta[n]
            print("%-64s %13s %11d  NEW   vgpr %s agpr %s sgpr %s scratch %s B lds(static) %s vgpr_spill %s sgpr_spill %s"
                  % (demangle(n), '-', len(tree[n]), m['.vgpr_count'], m['.agpr_count'], m['.sgpr_count'], m['.private_segment_fixed_size'],
                     m['.group_segment_fixed_size'], m['.vgpr_spill_count'], m['.sgpr_spill_count']))
    gone = [demangle(n) for n in parent if n not in tree]
    print("# kernels of the parent missing in the tree: %s" % (', '.join(gone) if gone else 'none'))


if __name__ == '__main__':
    main()
