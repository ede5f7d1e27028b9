"""Is the device code of a kernel, instruction for instruction, the same in two trees of the project?  No GPU needed.

Compiles the named sources of both trees for gfx950 with the flags of tools/kernel_resources.sh (the library's, without -Wall), takes
the code object out of each host object (llvm-objcopy: the .hip_fatbin section; clang-offload-bundler: the gfx950 entry),
disassembles it (llvm-objdump -d, without addresses and encodings) and compares the instruction lists per kernel instantiation.
Prints, per source, which kernels are identical and the instruction counts of those that are not; with --show N also the first N
differing blocks of every such kernel.  Exit status 1 when a kernel differs.

usage: python tools/kernel_code_compare.py TREE_A TREE_B [--show N] [source ...]      (sources without .hip; default: the four GNS
       backward / grid-per-workgroup sources)"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get('ROCM_LLVM', '/opt/rocm/llvm/bin')
FLAGS = '-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-slp-vectorize -ffp-contract=off -Wno-unused-function'.split()
DEFAULT = ['gns_backward', 'gns_backward_split', 'gns_gridwg', 'gns_gridwg_bwd']


def kernels(tree, source, tmp, tag):
    """name -> instruction list of every kernel of one source of one tree (the compile was started by the caller)"""
    base = os.path.join(tmp, f'{tag}_{source}')
    subprocess.run([f'{LLVM}/llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', base + '.o', base + '.fatbin'], check=True)
    subprocess.run([f'{LLVM}/clang-offload-bundler', '--type=o', '--unbundle', f'--input={base}.fatbin',
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--output={base}.co'], check=True, stderr=subprocess.DEVNULL)
    text = subprocess.run([f'{LLVM}/llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', base + '.co'], check=True,
                          capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'^[0-9a-f]* ?<(\S+)>:', line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r'\s*//.*$', '', line).strip())
    return out


def main(argv):
    show = 0
    if '--show' in argv:
        i = argv.index('--show')
        show = int(argv[i + 1])
        del argv[i:i + 2]
    if len(argv) < 2:
        sys.exit(__doc__)
    trees, sources = argv[:2], argv[2:] or DEFAULT
    tmp = tempfile.mkdtemp()
    jobs = []
    for tag, tree in zip('ab', trees):
        for s in sources:
            jobs.append(subprocess.Popen(['hipcc', *FLAGS, '-c', s + '.hip', '-o', os.path.join(tmp, f'{tag}_{s}.o')],
                                         cwd=os.path.join(tree, 'opf-graph-neural-solver_amd', 'csrc'), stderr=subprocess.DEVNULL))
    if any(j.wait() != 0 for j in jobs):
        sys.exit('a compile failed')
    total = same_total = 0
    for s in sources:
        a, b = kernels(trees[0], s, tmp, 'a'), kernels(trees[1], s, tmp, 'b')
        names = dict(zip(a, subprocess.run(['c++filt', *a], capture_output=True, text=True).stdout.split('\n')))
        same = [k for k in a if a[k] == b.get(k)]
        total, same_total = total + len(a), same_total + len(same)
        print(f'{s}.hip: {len(same)} of {len(a)} kernels identical')
        for k in a:
            name = names[k].replace('(anonymous namespace)::', '').split('(')[0].replace('void ', '')
            if k in same:
                print(f'  identical  {name}  ({len(a[k])} instructions)')
                continue
            print(f'  differs    {name}  {len(a[k])} -> {len(b.get(k, []))}')
            ops = [o for o in difflib.SequenceMatcher(None, a[k], b.get(k, []), autojunk=False).get_opcodes() if o[0] != 'equal']
            for o in ops[:show]:
                print('\n'.join(['    @ ' + str(o[1])] + ['    - ' + x for x in a[k][o[1]:o[2]]] + ['    + ' + x for x in b[k][o[3]:o[4]]]))
    print(f'{same_total} of {total} kernels identical')
    return 0 if same_total == total else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
