#!/usr/bin/env python3
"""Table of the GPU kernels in the objects of a library build, and the difference between two builds.

    python tools/kernel_table.py deepsolid_amd/csrc/build                 # one line per (object, kernel)
    python tools/kernel_table.py OLD_BUILD_DIR NEW_BUILD_DIR              # what a change of the host code did to the kernels
    python tools/kernel_table.py --bytes OLD_BUILD_DIR NEW_BUILD_DIR      # ... also the kernels of equal size whose code bytes differ

Per kernel: code bytes, VGPRs, AGPRs, SGPRs, scratch bytes, LDS bytes -- read from the symbol table and the metadata note of every
object's gfx950 code object (no disassembly; --bytes also hashes each kernel's code bytes).  The comparison ignores which object a kernel is in; it reports the kernels that
appear or disappear, the ones whose registers / scratch / LDS differ (none are expected from a move of host code), the ones whose
code bytes differ (possible: device functions are internalised per unit and the inliner sees other callers), and the kernels that
sit in more objects than before (the runtime keeps whichever registration comes first; the one-build table shows every home).  All
copies of a kernel are compared.  Exit status 1 when names or resources differ or a kernel gains a home."""
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/lib/llvm/bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--' + os.environ.get('ARCH', 'gfx950')
DIGEST = {}     # kernel symbol -> digests of its code bytes over the objects of the build being read (--bytes)
FIELDS = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels_of(obj, tmp):
    """{kernel symbol: (code bytes, vgpr, agpr, sgpr, scratch, lds)} of one host object"""
    fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'code.co')
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    run(os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, obj)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return {}
    run(os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET, '--input=' + fat, '--output=' + co)
    size = {}
    text = None                        # (address, file offset) of .text: where a symbol's bytes are
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-SW', co).splitlines():
        m = re.match(r'\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)', line)
        if m:
            text = (int(m.group(1), 16), int(m.group(2), 16))
    data = open(co, 'rb').read()
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '-sW', co).splitlines():
        p = line.split()
        if len(p) == 8 and p[3] == 'FUNC':
            size[p[7]] = int(p[2])
            if text:
                off = int(p[1], 16) - text[0] + text[1]
                DIGEST.setdefault(p[7], set()).add(hashlib.sha1(data[off:off + int(p[2])]).hexdigest()[:12])
    # the note is YAML: an entry of amdhsa.kernels opens with "  - .field:" and keeps its own fields at that depth
    out, cur, out_entries = {}, None, []
    for line in run(os.path.join(LLVM, 'llvm-readelf'), '--notes', co).splitlines():
        m = re.match(r'^  (- |  )(\.\w+):\s*(\S+)\s*$', line)
        if not m:
            continue
        if m.group(1) == '- ':
            cur = {}
            out_entries.append(cur)
        if cur is not None:
            cur[m.group(2)] = m.group(3)
    for e in out_entries:
        if '.name' in e and all(f in e for f in FIELDS):
            out[e['.name']] = (size.get(e['.name'], -1),) + tuple(int(e[f]) for f in FIELDS)
    return out


def table(build_dir):
    """{kernel: [(object, resources), ...]} over the objects of a build directory"""
    tab = {}
    DIGEST.clear()
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(build_dir, '*.o'))):
            for k, v in kernels_of(obj, tmp).items():
                tab.setdefault(k, []).append((os.path.basename(obj), v))
    return tab, {k: sorted(v) for k, v in DIGEST.items()}


def demangle(names):
    """readable names where a demangler is installed, the symbols themselves otherwise"""
    tool = shutil.which('llvm-cxxfilt', path=LLVM) or shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    if not names or not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input='\n'.join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def internal_linkage(sym):
    """whether a mangled name is that of a `static` function in a namespace (clang marks its source name with an L)"""
    m = re.match(r'_ZN', sym)
    i = 3 if m else len(sym)
    while i < len(sym):
        if sym[i] == 'L' and sym[i + 1:i + 2].isdigit():
            return True
        n = re.match(r'\d+', sym[i:])
        if not n:
            return False
        i += len(n.group()) + int(n.group())
    return False


def main(argv):
    same_bytes = '--bytes' in argv
    argv = [a for a in argv if a != '--bytes']
    if len(argv) == 2:
        tab, _ = table(argv[1])
        nice = demangle(sorted(tab))
        print('object\tcode\tvgpr\tagpr\tsgpr\tscratch\tlds\tkernel')
        for k in sorted(tab):
            for obj, v in tab[k]:
                print(obj + '\t' + '\t'.join(str(x) for x in v) + '\t' + nice[k])
        return 0
    if len(argv) != 3:
        print(__doc__)
        return 2
    (old, dig_old), (new, dig_new) = table(argv[1]), table(argv[2])
    nice = demangle(sorted(set(old) | set(new)))
    bad = 0
    print('kernels: %d before, %d after' % (len(old), len(new)))
    for k in sorted(set(old) - set(new)):
        print('GONE     ', nice[k]); bad = 1
    for k in sorted(set(new) - set(old)):
        print('NEW      ', nice[k]); bad = 1
    for k in sorted(set(old) & set(new)):
        a, b = sorted({v for _, v in old[k]}), sorted({v for _, v in new[k]})       # every copy of the kernel, not one home
        if [v[1:] for v in a] != [v[1:] for v in b]:
            print('RESOURCES', nice[k], 'vgpr/agpr/sgpr/scratch/lds', [v[1:] for v in a], '->', [v[1:] for v in b]); bad = 1
        elif a != b:
            print('CODE     ', nice[k], [v[0] for v in a], '->', [v[0] for v in b], 'bytes')
        elif same_bytes and dig_old.get(k) != dig_new.get(k):
            print('BYTES    ', nice[k], 'same size, other code bytes')
    # rule: the kernels with more than one home must not become more, and none of them may gain a home.  A `static` kernel is a
    # kernel of its own in every object that includes its header (no registration shadows another): reported, not counted
    dup_old, dup_new = ({k for k in t if len(t[k]) > 1} for t in (old, new))
    print('kernels in more than one object: %d before, %d after' % (len(dup_old), len(dup_new)))
    for k in sorted(dup_new):
        n0, n1 = len(old.get(k, ())), len(new[k])
        if n1 > n0 and internal_linkage(k):
            print('STATIC, %d -> %d OBJECTS' % (n0, n1), nice[k])
        elif n1 > n0:
            print('MORE HOMES, %d -> %d OBJECTS' % (n0, n1), nice[k], ' '.join(o for o, _ in new[k])); bad = 1
    return bad


if __name__ == '__main__':
    sys.exit(main(sys.argv))
