"""Developer helper: VGPR / AGPR / spill / LDS counts of the kernels in a gfx950 device assembly file (`hipcc ... --save-temps`, or
the file's Makefile flags plus `--cuda-device-only -S`), and a digest of each kernel's instruction text: two builds whose digests
agree run the same instruction stream for that kernel, whatever else their files hold.
usage: python tools/kernel_regs.py <file.s> [name-substring]
Digest: the text from the kernel's label to its .Lfunc_end, comments stripped, .loc / .cfi / .p2align lines dropped, block
labels .LBB<n>_ rewritten to .LBB_ (n is the function's index in its file) and the kernel's own name to a placeholder (the text
holds its .amdhsa_kernel block and section name), so that a kernel whose template argument list changed still compares."""
import hashlib
import re
import sys


def digest(asm, name):
    m = re.search(r'^%s:.*?^\.Lfunc_end\d+:' % re.escape(name), asm, re.M | re.S)
    if not m:
        return '-' * 12
    lines = []
    for ln in m.group(0).split('\n'):
        ln = re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].split('//')[0]).replace(name, '<kernel>').strip()
        if ln and not re.match(r'\.(loc|cfi_\w+|p2align)\b', ln) and not ln.startswith('.Lfunc_end'):
            lines.append(' '.join(ln.split()))
    return hashlib.sha1('\n'.join(lines).encode()).hexdigest()[:12]


def kernels(asm):
    """[(mangled name, agpr, vgpr, spilled vgprs, static LDS bytes, digest)] of every kernel of the file"""
    out = []
    for blk in asm.split('  - .agpr_count:')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        f = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, blk).group(1))
        out.append((name, int(blk.split()[0]), f('vgpr_count'), f('vgpr_spill_count'), f('group_segment_fixed_size'), digest(asm, name)))
    return out


if __name__ == '__main__':
    for name, agpr, vgpr, spill, lds, dg in kernels(open(sys.argv[1]).read()):
        if len(sys.argv) > 2 and sys.argv[2] not in name:
            continue
        print(name[:70], 'agpr', agpr, 'vgpr', vgpr, 'spill', spill, 'lds', lds, 'digest', dg)
