"""Build libpacoh_gp.so (the C-ABI library of hand-written HIP kernels) in-tree for gfx950.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the resulting
.so travels to the GPU box with the repository snapshot (it is git-ignored, not gpurun-ignored).
"""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')
OBJ_DIR = os.path.join(HERE, 'build')
LIB_DIR = os.path.join(HERE, 'lib')
LIB_PATH = os.path.join(LIB_DIR, 'libpacoh_gp.so')
SOURCES = ['gp_small.hip', 'gp_mfma.hip', 'gp_reg.hip', 'gp_fwd_reg.hip', 'gp_reg_matern.hip', 'map_persist.hip', 'map_task.hip', 'map_wide.hip', 'gram.hip', 'dense.hip', 'dense_mfma.hip', 'dense_ll.hip', 'dense_trtri_ll.hip', 'dense_grad_mfma.hip', 'dense_gp.hip', 'mlp.hip', 'mlp_mfma.hip', 'mlp_fused.hip', 'mlp_layers.hip', 'misc.hip', 'distinct.hip', 'svgd_imq.hip', 'vi_full.hip', 'comm.hip', 'predictive.hip', 'acq.hip', 'mvn_sample.hip', 'gp_loo.hip', 'gp_cond.hip', 'gp_path.hip']
ARCH = 'gfx950'
# per-source flags.  mlp_fused.hip: the compiler's automatic v_pk_fma_f32 / v_pk_add_f32 pairing costs the MFMA-paced backward
# kernel 11-13 % (240 -> 213 us at cfg #3; packed fp32 issues at half rate and needs extra moves) -- the GP kernel is the
# opposite case (5 % slower without it), so this is not a global flag
PER_FILE_FLAGS = {'mlp_fused.hip': ['-fno-slp-vectorize']}
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=' + ARCH, '-Wno-pass-failed', '-Wno-unused-value']


def _hipcc():
    for cand in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found: libpacoh_gp.so cannot be built')


def source_hash():
    """sha256 (first 16 hex digits) over the kernel sources (csrc/*.hip, *.h, include/pacoh_gp.h): the committed PMC traffic profiles
    record the hash of the sources they were taken on, and bench.py marks a `traffic` figure stale when the sources have moved on"""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hip', '.h', '.inc')))
    for path in files + [os.path.join(INCLUDE, 'pacoh_gp.h')]:
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _deps_mtime():
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.h', '.inc'))]
    hdrs.append(os.path.join(INCLUDE, 'pacoh_gp.h'))
    return max(os.path.getmtime(h) for h in hdrs)


def build_library(force=False, verbose=True, variant=None, extra_flags=()):
    """Compile every .hip source for gfx950 and link the shared library.  Returns its path.
    variant / extra_flags: an experimental build next to the product library (lib/libpacoh_gp_<variant>.so, selected at run time
    with PACOH_LIB=<path>) compiled with additional flags, e.g. a diagnostic stamps build: --variant lst -DPACOH_LL_STAMPS=1."""
    obj_dir = OBJ_DIR if variant is None else OBJ_DIR + '_' + variant
    lib_path = LIB_PATH if variant is None else os.path.join(LIB_DIR, 'libpacoh_gp_%s.so' % variant)
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = _hipcc()
    hdr_m = _deps_mtime()
    sources = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    jobs = []
    for src in sources:
        sp = os.path.join(CSRC, src)
        op = os.path.join(obj_dir, src.replace('.hip', '.o'))
        stale = force or not os.path.exists(op) or os.path.getmtime(op) < max(os.path.getmtime(sp), hdr_m)
        if stale:
            jobs.append((sp, op))

    def compile_one(job):
        sp, op = job
        cmd = [hipcc] + FLAGS + PER_FILE_FLAGS.get(os.path.basename(sp), []) + list(extra_flags) + ['-I', INCLUDE, '-c', sp, '-o', op]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed for %s:\n%s' % (sp, r.stdout[-4000:]))
        return sp

    if jobs:
        if verbose:
            print('[pacoh build] compiling %d source(s) for %s' % (len(jobs), ARCH), file=sys.stderr)
        with ThreadPoolExecutor(max_workers=min(6, len(jobs))) as ex:
            list(ex.map(compile_one, jobs))
    objs = [os.path.join(obj_dir, s.replace('.hip', '.o')) for s in sources]
    if jobs or not os.path.exists(lib_path) or os.path.getmtime(lib_path) < max(os.path.getmtime(o) for o in objs):
        cmd = [hipcc, '-shared', '-fPIC', '--offload-arch=' + ARCH, '-o', lib_path] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError('link failed:\n%s' % r.stdout[-4000:])
    return lib_path


def build_asan_shim(verbose=False):
    """Host-side AddressSanitizer build (sanitizers run on the CPU build only): every source compiled --cuda-host-only with
    -fsanitize=address into lib/libpacoh_gp_asan_host.so (no device code: it cannot launch anything) and tests/asan/abi_shim.cpp
    linked against it.  Returns the path of the shim executable (tests/test_abi.py runs it)."""
    obj_dir = OBJ_DIR + '_asan_host'
    os.makedirs(obj_dir, exist_ok=True)
    os.makedirs(LIB_DIR, exist_ok=True)
    hipcc = _hipcc()
    san = ['-O1', '-g', '-std=c++17', '-fPIC', '--offload-arch=' + ARCH, '--cuda-host-only', '-fsanitize=address',
           '-fno-omit-frame-pointer', '-Wno-pass-failed', '-Wno-unused-value', '-I', INCLUDE]
    sources = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdr_m = _deps_mtime()

    def compile_one(src):
        sp, op = os.path.join(CSRC, src), os.path.join(obj_dir, src.replace('.hip', '.o'))
        if os.path.exists(op) and os.path.getmtime(op) >= max(os.path.getmtime(sp), hdr_m):
            return op
        r = subprocess.run([hipcc] + san + ['-c', sp, '-o', op], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc (ASan host build) failed for %s:\n%s' % (sp, r.stdout[-4000:]))
        return op

    with ThreadPoolExecutor(max_workers=6) as ex:
        objs = list(ex.map(compile_one, sources))
    # a host-only object still refers to its (absent) device code object as __hip_fatbin_<hash>: empty stand-ins, which the HIP
    # runtime only records at load time (code objects are parsed on the first launch, and this library never launches)
    nm = subprocess.run(['nm', '-u'] + objs, stdout=subprocess.PIPE, text=True).stdout
    syms = sorted({ln.split()[-1] for ln in nm.splitlines() if '__hip_fatbin_' in ln})
    stub_c = os.path.join(obj_dir, 'fatbin_stubs.c')
    with open(stub_c, 'w') as fh:
        fh.write(''.join('__attribute__((aligned(4096))) const char %s[64] = {0};\n' % sym for sym in syms))
    stub_o = stub_c[:-2] + '.o'
    subprocess.run(['gcc', '-fPIC', '-c', stub_c, '-o', stub_o], check=True)
    objs = objs + [stub_o]
    lib_path = os.path.join(LIB_DIR, 'libpacoh_gp_asan_host.so')
    r = subprocess.run([hipcc, '-shared', '-fPIC', '-fsanitize=address', '-o', lib_path] + objs,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError('ASan host link failed:\n%s' % r.stdout[-4000:])
    shim_src = os.path.join(os.path.dirname(HERE), 'tests', 'asan', 'abi_shim.cpp')
    shim = os.path.join(obj_dir, 'abi_shim')
    r = subprocess.run([hipcc, '-x', 'c++', '-O1', '-g', '-std=c++17', '-fsanitize=address', '-fno-omit-frame-pointer', '-I', INCLUDE,
                        shim_src, '-x', 'none', lib_path, '-Wl,-rpath,' + LIB_DIR, '-o', shim],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError('ASan shim build failed:\n%s' % r.stdout[-4000:])
    if verbose:
        print('[pacoh build] ASan host shim:', shim, file=sys.stderr)
    return shim


if __name__ == '__main__':
    # python -m meta_learning_pacoh_amd._build [--force] [--variant NAME -DFLAG ...]
    argv = sys.argv[1:]
    variant = argv[argv.index('--variant') + 1] if '--variant' in argv else None
    flags = [a for a in argv if a.startswith(('-D', '-f', '-m'))]
    print(build_library(force='--force' in argv, variant=variant, extra_flags=flags))
