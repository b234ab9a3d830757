"""Host side of the transition-block entry convolution (no GPU, no launch): ``um_conv2d_entry_supported`` is a pure function of the
geometry, offered for 3x3 / stride 2 / pad 1 only, and ``um_conv2d_entry_fwd`` / ``um_nhwc_instance_norm_sc`` answer bad arguments
with error codes."""
import ctypes
import itertools

from unimatch_amd import _abi


def test_entry_support_is_a_pure_function_of_the_geometry():
    """Over a sweep of geometries: the same answer on every call (no environment, no device state), a tile width on or off as a
    whole, and never for stride 1, 1x1 / 5x1 main kernels, other paddings, cin % 32 != 0 or a bad mode."""
    lib = _abi.load()
    sup = lib.um_conv2d_entry_supported
    sizes = [(256, 384), (128, 192), (64, 96), (68, 132), (60, 100), (22, 60), (31, 45), (15, 25), (8, 12), (3, 3), (1, 1), (2, 7)]
    seen = {0: 0, 1: 0}
    for (h, w), (cin, cout), mode in itertools.product(sizes, ((64, 96), (96, 128), (64, 64), (128, 128), (32, 96), (96, 192)), (0, 1)):
        s = sup(h, w, cin, cout, 3, 3, 2, 1, 1, mode)
        assert s in (0, 1)
        seen[s] += 1
        assert all(sup(h, w, cin, cout, 3, 3, 2, 1, 1, mode) == s for _ in range(3))
        assert s == sup(256, 384, cin, cout, 3, 3, 2, 1, 1, mode), (h, w, cin, cout)      # depends on the widths only
        # both outputs of the launch number their statistics parts alike: one per 128 output pixels
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        assert lib.um_conv_stats_parts(h, w, cout, 3, 3, 2, 1, 1) == lib.um_conv_stats_parts(h, w, cout, 1, 1, 2, 0, 0) == (ho * wo + 127) // 128
        assert sup(h, w, cin, cout, 3, 3, 1, 1, 1, mode) == 0                             # stride 1
        assert sup(h, w, cin, cout, 1, 1, 2, 0, 0, mode) == 0                             # 1x1 main kernel
        assert sup(h, w, cin, cout, 5, 1, 2, 2, 0, mode) == 0 and sup(h, w, cin, cout, 1, 5, 2, 0, 2, mode) == 0
        assert sup(h, w, cin, cout, 3, 3, 2, 0, 0, mode) == 0 and sup(h, w, cin, cout, 3, 3, 2, 1, 0, mode) == 0
        assert sup(h, w, cin, cout, 3, 3, 4, 1, 1, mode) == 0
    assert seen[0] > 0
    assert sup(256, 384, 64, 64, 3, 3, 2, 1, 1, 0) == 0                                  # a 64-wide tile has no entry twin
    assert sup(0, 32, 64, 96, 3, 3, 2, 1, 1, 0) == 0 and sup(64, 0, 64, 96, 3, 3, 2, 1, 1, 0) == 0
    assert sup(64, 96, 48, 96, 3, 3, 2, 1, 1, 0) == 0 and sup(64, 96, 80, 96, 3, 3, 2, 1, 1, 0) == 0        # cin % 32
    assert sup(64, 96, 160, 128, 3, 3, 2, 1, 1, 0) == 0                                  # more input channels than statistics fit
    assert sup(64, 96, 64, 96, 3, 3, 2, 1, 1, 2) == 0 and sup(64, 96, 64, 96, 3, 3, 2, 1, 1, -1) == 0       # mode
    assert sup(64, 96, 64, 98, 3, 3, 2, 1, 1, 0) == 0                                    # cout % 4


def test_entry_points_reject_bad_arguments_without_a_launch():
    lib = _abi.load()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    conv = lib.um_conv2d_entry_fwd
    ok_geo = (1, 64, 96, 64, 96, 3, 3, 2, 1, 1, 10, 0, None)                    # batch .. stream
    ptrs = [fake] * 10                     # u, ustats, s_planes, w_planes, w2_planes, bias2, out_t, out_d, stats_t, stats_d
    for i in (0, 1, 2, 3, 4, 6, 7):        # the projection's bias and the statistics outputs are optional
        p = list(ptrs)
        p[i] = None
        assert conv(*p, *ok_geo) == -1, i
        assert b'um_conv2d_entry_fwd' in lib.um_last_error_string()
    for i in (0, 2, 3, 4, 5, 6, 7):
        p = list(ptrs)
        p[i] = odd
        assert conv(*p, *ok_geo) == -1 and b'aligned' in lib.um_last_error_string(), i
    assert conv(*ptrs, 0, 64, 96, 64, 96, 3, 3, 2, 1, 1, 10, 0, None) == -1       # batch
    assert conv(*ptrs, 1, 64, 96, 64, 96, 3, 3, 2, 1, 1, 15, 0, None) == -1       # wshift
    # geometries the entry kernel does not serve: an error, not another kernel and not a wrong answer
    for geo in ((64, 96, 64, 96, 3, 3, 1, 1, 1), (64, 96, 64, 96, 1, 1, 2, 0, 0), (64, 96, 64, 96, 5, 1, 2, 2, 0),
                (64, 96, 48, 96, 3, 3, 2, 1, 1), (64, 96, 64, 64, 3, 3, 2, 1, 1), (64, 96, 64, 96, 3, 3, 2, 0, 0)):
        assert lib.um_conv2d_entry_supported(*geo, 0) == 0
        assert conv(*ptrs, 1, *geo, 10, 0, None) == -2, geo
        assert b'um_conv2d_entry_supported' in lib.um_last_error_string()
    assert conv(*ptrs, 1, 64, 96, 64, 96, 3, 3, 2, 1, 1, 10, 2, None) == -2       # mode
    assert conv(*ptrs, 4096, 1024, 1024, 64, 96, 3, 3, 2, 1, 1, 10, 0, None) == -4      # beyond the kernel's 32-bit addressing

    norm = lib.um_nhwc_instance_norm_sc
    ws = lib.um_nhwc_norm_sc_workspace_bytes(2, 512, 64)
    assert ws == lib.um_nhwc_norm_workspace_bytes(2, 512, 64) + 2 * 2 * 64 * 4 and lib.um_nhwc_norm_sc_workspace_bytes(0, 512, 64) == 0
    tail = (0, None)                                                             # mode, stream
    assert norm(fake, fake, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, None, 4) == -1       # no shortcut statistics
    assert b'um_nhwc_instance_norm_sc' in lib.um_last_error_string()
    assert norm(fake, fake, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 0) == -1       # no parts
    assert norm(fake, None, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # no fp32 shortcut
    assert norm(fake, None, fake, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # planes shortcut
    assert norm(fake, fake, None, fake, None, 2, 512, 64, 1e-5, 0, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # normalize = 0
    assert norm(None, fake, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # no input
    assert norm(fake, fake, None, None, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # no output
    assert norm(fake, fake, None, fake, None, 2, 512, 60, 1e-5, 1, 1, fake, 4, fake, ws, *tail, fake, 4) == -1       # channels % 8
    # the workspace of the plain entry is one statistics set short
    assert norm(fake, fake, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws - 4, *tail, fake, 4) == -3
    assert norm(fake, fake, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, None, 0, *tail, fake, 4) == -3
    assert b'workspace' in lib.um_last_error_string()
    # the plain entry keeps its signature and its answers
    plain = lib.um_nhwc_instance_norm
    assert plain(None, None, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, fake, ws, *tail) == -1
    assert plain(fake, None, None, fake, None, 2, 512, 64, 1e-5, 1, 1, fake, 4, None, 0, *tail) == -3
    assert b'um_nhwc_instance_norm:' in lib.um_last_error_string()
    # the census has no new id: the entry launch counts as the generic kernel
    assert _abi.CENSUS['conv_generic'] == 12 and len(_abi.CENSUS) == 15 and lib.um_census_count(14) >= 0 and lib.um_census_count(15) == -1


def test_the_build_guards_the_entry_kernels_registers():
    """conv_entry_kernel<Fp16, 2, 4> sits at the register limit of two workgroups per CU.  The build reads the compiler's resource
    report of conv.hip and refuses a kernel that spills or loses occupancy; the report it accepted lies next to the object."""
    import os

    import pytest

    from unimatch_amd import build
    sample = '\n'.join([
        'remark: conv.hip:636:0: Function Name: _Z17conv_entry_kernelI4Fp16Li2ELi4EEv8ConvArgs13ConvEntryArgs [-Rpass-analysis=kernel-resource-usage]',
        'remark: conv.hip:636:0:     VGPRs: 256 [-Rpass-analysis=kernel-resource-usage]',
        'remark: conv.hip:636:0:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]',
        'remark: conv.hip:636:0:     Occupancy [waves/SIMD]: 2 [-Rpass-analysis=kernel-resource-usage]'])
    rep = build.parse_resource_report(sample)
    assert rep == {'_Z17conv_entry_kernelI4Fp16Li2ELi4EEv8ConvArgs13ConvEntryArgs': {'VGPRs': 256, 'ScratchSize': 0, 'Occupancy': 2}}
    build.check_resources('conv.hip', rep)
    for field, bad in (('ScratchSize', 16), ('Occupancy', 1)):
        with pytest.raises(RuntimeError, match='conv_entry_kernel'):
            build.check_resources('conv.hip', {k: dict(v, **{field: bad}) for k, v in rep.items()})
    with pytest.raises(RuntimeError, match='nothing to check'):
        build.check_resources('conv.hip', {})
    # what the build of this tree accepted
    path = os.path.join(os.path.dirname(build.LIB), '_obj', 'conv.resources.txt')
    assert os.path.exists(path), 'python -m unimatch_amd.build writes the resource report of conv.hip next to its object'
    real = {k: v for k, v in build.parse_resource_report(open(path).read()).items() if 'conv_entry_kernel' in k}
    assert len(real) == 4, sorted(real)                                          # NT = 3, 4 in both arithmetics
    for name, r in real.items():
        assert r['ScratchSize'] == 0 and r['Occupancy'] >= 2 and r['VGPRs'] <= 256, (name, r)
