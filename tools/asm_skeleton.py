"""Memory skeleton of the kernels in a HIP source (compile only, no GPU): per kernel, in program order, the loads, the
stores, the s_waitcnt's, the labels and the branches -- what shows how many dependent trips to memory a kernel makes.
    python tools/asm_skeleton.py point_dae_amd/csrc/block.hip [name-substring]
The flags are FLAGS of point_dae_amd/csrc/Makefile.  tests/test_block_codegen_cpu.py imports the parser."""
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def makefile_flags():
    """FLAGS of the csrc Makefile with $(ARCH) expanded."""
    text = open(os.path.join(ROOT, 'point_dae_amd', 'csrc', 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    flags = re.search(r'^FLAGS\s*\?=\s*(.+)$', text, re.M).group(1)
    return flags.replace('$(ARCH)', arch).split()


def device_asm(src):
    """The device-side assembly of `src` as text."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        subprocess.run([HIPCC] + makefile_flags() + ['--cuda-device-only', '-S', os.path.abspath(src), '-o', out],
                       check=True, capture_output=True)
        return open(out).read()


def demangle(names):
    out = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout
    return dict(zip(names, out.split('\n')))


def kernels(asm):
    """{demangled name: {'body': [instruction lines], 'private': bytes, 'symbol': mangled}} of every kernel."""
    private = {}
    for blk in re.split(r'\n  - \.agpr_count:', asm)[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        private[name] = int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', blk).group(1))
    pretty = demangle(list(private))
    found = {}
    for sym in private:
        m = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(sym), asm, re.M | re.S)
        body = [ln.split(';')[0].strip() for ln in m.group(1).split('\n')]
        found[pretty[sym]] = {'body': [ln for ln in body if ln], 'private': private[sym], 'symbol': sym}
    return found


MEM = re.compile(r'^(global_load|flat_load|scratch_load|buffer_load|global_store|flat_store|scratch_store|global_atomic|'
                 r'flat_atomic|s_load|s_waitcnt|s_cbranch|s_branch|s_barrier|ds_read|ds_write|\.LBB)')


def skeleton(body):
    return [ln for ln in body if MEM.match(ln)]


def loops(body):
    """(first, last) instruction index of every loop: a branch back to a label above it."""
    at = {ln[:-1]: i for i, ln in enumerate(body) if ln.startswith('.LBB') and ln.endswith(':')}
    spans = []
    for i, ln in enumerate(body):
        m = re.match(r's_c?branch\S*\s+(\.LBB\S+)', ln)
        if m and at.get(m.group(1), i + 1) <= i:
            spans.append((at[m.group(1)], i))
    return spans


if __name__ == '__main__':
    want = sys.argv[2] if len(sys.argv) > 2 else ''
    for name, k in kernels(device_asm(sys.argv[1])).items():
        if want not in name:
            continue
        sk = skeleton(k['body'])
        print('== %s\n   private segment %d, %d flat loads, %d loops' % (
            name.split('(')[0], k['private'], sum(ln.startswith('flat_load') for ln in sk), len(loops(k['body']))))
        for ln in sk:
            print('     ' + ln)
