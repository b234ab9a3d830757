"""Build recipe for the HIP extension: ``hipcc --offload-arch=gfx950`` -> ``unimatch_amd/libunimatch_hip.so``.

In-tree on purpose: the built ``.so`` travels with a snapshot of the repository (it is git-ignored, so the
history stays source-only).  hipcc cross-compiles without a GPU.  Usage: ``python -m unimatch_amd.build``.
"""
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libunimatch_hip.so')
SOURCES = ['capi.hip', 'global_match.hip', 'window_attn.hip', 'local_ops.hip', 'linear.hip', 'ffn.hip', 'conv.hip', 'nhwc_ops.hip', 'norm_ops.hip', 'upsample.hip',
           'rccl_gather.hip', 'local_corr_mfma.hip', 'aliases.hip', 'probe.hip', 'video.hip', 'metrics.hip', 'prepost.hip', 'visualize.hip', 'geometry.hip', 'match_stats.hip',
           'interp.hip', 'depth_multi.hip', 'fusion.hip', 'tsdf_mesh.hip']
# hardware micro-benchmarks (um_debug_*): diagnostic builds only, never in the shipped library
DIAG_SOURCES = ['microbench.hip']
HEADERS = ['common.h', 'planes.h', 'timing.h', 'local_pixel.h', 'tsdf_grid.h', os.path.join('..', '..', 'include', 'unimatch_hip.h')]
# per-file extras: the FFN kernel's hand-placed scalar VALU stream must not be re-packed into v_pk_* by the SLP vectorizer
EXTRA_FLAGS = {'ffn.hip': ['-fno-slp-vectorize'], 'global_match.hip': ['-fno-slp-vectorize', '-mllvm', '-amdgpu-mfma-vgpr-form', '-Wno-inline-asm'], 'window_attn.hip': ['-fno-slp-vectorize'],
               'linear.hip': ['-fno-slp-vectorize'],
               # the post-processing and metric kernels round every product and sum separately, as the reference's NumPy / ATen steps do
               'video.hip': ['-ffp-contract=off'],
               # ... and take IEEE square roots and quotients (hipcc's default, stated because the results depend on it)
               'metrics.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # the resize / normalise kernels are compared bit for bit with a host restatement of the same operation order
               'prepost.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # ... and so are the colour-map kernels (normalisation of a scalar map, the percentile's interpolation)
               'visualize.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # ... and the consistency / point-cloud kernels follow their host restatement operation by operation
               'geometry.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # ... and the frame-synthesis kernels theirs: bit for bit, integer accumulators included
               'interp.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # ... and the TSDF fusion kernels theirs: the running averages of a voxel, bit for bit
               'fusion.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # ... and the mesh vertices of the volume are, on the axis edges, bit for bit the points of fusion.hip
               'tsdf_mesh.hip': ['-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt'],
               # the confidence kernel's final quotients are IEEE: a row with one key gives max_prob = l / l = 1 exactly
               'match_stats.hip': ['-fno-slp-vectorize', '-fhip-fp32-correctly-rounded-divide-sqrt', '-Wno-inline-asm']}
# kernels that sit at the register limit of their occupancy (conv_entry_kernel<Fp16, 2, 4>: all 256 VGPRs of two workgroups per CU): the
# build reads the compiler's resource report for these sources and fails if a named kernel spills to scratch or loses occupancy,
# instead of shipping a silently slower kernel.  source -> {substring of the mangled kernel name: minimum waves per SIMD}
RESOURCE_GUARDS = {'conv.hip': {'conv_entry_kernel': 2},
                   # the plane sweep (K7), plain and with statistics: no scratch in any of the four kernels, three waves per SIMD as before the statistics
                   'local_ops.hip': {'depth_corr_softmax_kernel': 3, 'depth_corr_softmax_box_kernel': 3, 'depth_corr_softmax_stats_kernel': 3,
                                     'depth_corr_softmax_box_stats_kernel': 3},
                   # the multi-view plane sweep: the same table and the same three waves as K7's box form, no scratch
                   # (the row-table kernels are the same two bodies with another operand addressing)
                   'depth_multi.hip': {'depth_multi_box_kernel': 3, 'depth_multi_gather_kernel': 3,
                                       'depth_multi_rows_box_kernel': 3, 'depth_multi_rows_gather_kernel': 3},
                   # memory-bound per-pixel kernels: no scratch, and registers far below what would cost a wave
                   'geometry.hip': {'disp_consistency_kernel': 4, 'depth_consistency_kernel': 4, 'points_count_kernel': 4,
                                    'points_scan_kernel': 4, 'points_scatter_kernel': 4},
                   # the confidence kernel is laid out for two workgroups per CU (64 KB of LDS each in exact mode); the mutual check is per-pixel
                   'match_stats.hip': {'match_stats_kernel': 2, 'match_mutual_kernel': 4},
                   # per-pixel gather / scatter kernels: memory- and atomic-bound, no scratch (the times are indexed in the kernel arguments)
                   'interp.hip': {'image_warp_kernel': 4, 'flow_splat_kernel': 4, 'splat_normalize_kernel': 4, 'frame_synth_kernel': 4},
                   # memory-bound per-voxel kernels, as the per-pixel ones of geometry.hip: no scratch, no wave lost to registers
                   'fusion.hip': {'tsdf_integrate_kernel': 4, 'tsdf_points_count_kernel': 4, 'tsdf_points_scan_kernel': 4,
                                  'tsdf_points_scatter_kernel': 4},
                   # the marching-tetrahedra passes: per-voxel traversals of byte-sized codes, no scratch (the face pass keeps the vertex
                   # bases and masks of a cell's seven edge owners in registers)
                   'tsdf_mesh.hip': {'tsdf_mesh_cells_kernel': 4, 'tsdf_mesh_classify_kernel': 4, 'tsdf_mesh_scan_kernel': 4,
                                     'tsdf_mesh_vertices_kernel': 4, 'tsdf_mesh_faces_kernel': 4}}
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-gpu-rdc', '-Wno-unused-result']


def find_hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found: the HIP extension cannot be built')


def parse_resource_report(text):
    """``-Rpass-analysis=kernel-resource-usage`` remarks -> ``{mangled kernel name: {'VGPRs': n, 'ScratchSize': n, 'Occupancy': n, ...}}``."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark: .*?Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark: .*?\s{2,}([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def check_resources(src, report):
    """Raise when a guarded kernel of ``src`` (RESOURCE_GUARDS) is missing from the report, uses scratch or is below its occupancy."""
    for key, min_occ in RESOURCE_GUARDS.get(src, {}).items():
        hits = {k: v for k, v in report.items() if key in k}
        if not hits:
            raise RuntimeError(f'{src}: no resource report for {key}: the guard of unimatch_amd/build.py has nothing to check')
        for name, r in hits.items():
            if r.get('ScratchSize', -1) != 0 or r.get('Occupancy', 0) < min_occ:
                raise RuntimeError(f'{src}: {name} needs scratch {r.get("ScratchSize")} B/lane at occupancy {r.get("Occupancy")} '
                                   f'({r.get("VGPRs")} VGPRs): it was written for no scratch at {min_occ} waves per SIMD')


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 and link the shared library.  Returns the library path."""
    hipcc = find_hipcc()
    objdir = os.path.join(HERE, '_obj')
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS] + [os.path.abspath(__file__)]
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        # a guarded source's report is part of its build: an object without one (built before the guard, or cleaned) is compiled again
        if force or _stale(o, [s] + hdrs) or (src in RESOURCE_GUARDS and not os.path.exists(o[:-2] + '.resources.txt')):
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ['-c', s, '-o', o]
            if verbose:
                print(' '.join(cmd))
            if src in RESOURCE_GUARDS:
                done = subprocess.run(cmd + ['-Rpass-analysis=kernel-resource-usage', '-fno-caret-diagnostics'], cwd=CSRC, stderr=subprocess.PIPE, text=True)
                remarks = [ln for ln in done.stderr.splitlines() if 'kernel-resource-usage' in ln]
                sys.stderr.write('\n'.join(ln for ln in done.stderr.splitlines() if 'kernel-resource-usage' not in ln))
                if done.returncode != 0:
                    raise subprocess.CalledProcessError(done.returncode, cmd)
                try:
                    check_resources(src, parse_resource_report('\n'.join(remarks)))
                except RuntimeError:
                    os.remove(o)                     # not a usable object: the next build must compile (and check) it again
                    raise
                with open(o[:-2] + '.resources.txt', 'w') as f:
                    f.write('\n'.join(remarks) + '\n')
            else:
                subprocess.run(cmd, check=True, cwd=CSRC)
        objs.append(o)
    if force or _stale(LIB, objs):
        cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs + ['-ldl']
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True)
    return LIB


def build_variant(name, defines, verbose=False, only=None):
    """A diagnostic build ``unimatch_amd/_variants/lib<name>.so`` of the whole library with extra ``-D`` flags (A/B switches
    behind -DUM_DEBUG_SWITCHES, precision-budget experiments ...); load it with ``UM_LIB=<path>`` (tools/ab_bench.py).
    ``only``: source files the flags concern (``--only window_attn.hip,ffn.hip``) -- the other objects are the shipped build's
    (brought up to date first), which turns a 90 s variant build into a 10 s one."""
    hipcc = find_hipcc()
    objdir = os.path.join(HERE, '_variants', '_obj_' + name)
    os.makedirs(objdir, exist_ok=True)
    objs = []
    defines = list(defines) + ['-DUM_DIAGNOSTIC_BUILD']
    if only:
        build(verbose=verbose)
    for src in SOURCES + DIAG_SOURCES:
        if only and src not in only and src not in DIAG_SOURCES:
            objs.append(os.path.join(HERE, '_obj', src.replace('.hip', '.o')))
            continue
        o = os.path.join(objdir, src.replace('.hip', '.o'))
        cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + list(defines) + ['-c', os.path.join(CSRC, src), '-o', o]
        if verbose:
            print(' '.join(cmd))
        subprocess.run(cmd, check=True, cwd=CSRC)
        objs.append(o)
    lib = os.path.join(HERE, '_variants', f'lib{name}.so')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', lib] + objs + ['-ldl'], check=True)
    shutil.rmtree(objdir, ignore_errors=True)
    return lib


if __name__ == '__main__':
    if '--variant' in sys.argv:            # python -m unimatch_amd.build --variant NAME -DFOO=1 -DBAR
        i = sys.argv.index('--variant')
        only = sys.argv[sys.argv.index('--only') + 1].split(',') if '--only' in sys.argv else None
        print(build_variant(sys.argv[i + 1], [a for a in sys.argv[i + 2:] if a.startswith('-D')], verbose=True, only=only))
    else:
        print(build(force='--force' in sys.argv, verbose=True))
