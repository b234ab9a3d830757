"""Host side of the normalise-on-load convolution (no GPU, no launch): ``um_conv2d_norm_supported`` is a pure function of the
geometry that agrees with the kernel dispatch ``um_conv_stats_parts`` exposes, and the new entry points answer bad arguments with
error codes."""
import ctypes
import itertools

from unimatch_amd import _abi


def _patch_parts(h, w):
    return 2 * ((h + 7) // 8) * ((w + 31) // 32)


def test_norm_on_load_support_follows_the_patch_kernel_dispatch():
    """Over a sweep of geometries the on-load path is offered only where the 2-D patch kernel serves (its statistics parts are
    numbered 2 per 8 x 32 tile), never for strides, 1x1 / 5x1 kernels or maps under 3/4 tile coverage, and the answer is the
    same on every call (no environment, no device state)."""
    lib = _abi.load()
    sup, parts = lib.um_conv2d_norm_supported, lib.um_conv_stats_parts
    seen = {0: 0, 1: 0}
    sizes = [(256, 384), (128, 192), (64, 96), (32, 48), (16, 24), (68, 132), (34, 66), (17, 33), (60, 100), (30, 50), (15, 25),
             (22, 60), (30, 31), (15, 90), (40, 7), (8, 12), (8, 32), (9, 33), (47, 63)]
    for (h, w), c, mode in itertools.product(sizes, (64, 96, 128), (0, 1)):
        s = sup(h, w, c, c, 3, 3, 1, 1, 1, mode)
        assert s in (0, 1)
        seen[s] += 1
        assert all(sup(h, w, c, c, 3, 3, 1, 1, 1, mode) == s for _ in range(3))
        tiled = ((h + 7) // 8 * 8) * ((w + 31) // 32 * 32)
        by_rule = h * w >= 256 and 4 * h * w >= 3 * tiled                       # conv_pick's patch-kernel rule for 3x3 / 1 / 1
        if s:
            assert by_rule and parts(h, w, c, 3, 3, 1, 1, 1) == _patch_parts(h, w), (h, w, c)
        if not by_rule:
            assert s == 0 and parts(h, w, c, 3, 3, 1, 1, 1) == (h * w + 127) // 128, (h, w, c)
        # a tile width is on or off as a whole: the answer depends on the geometry only through the dispatch
        assert s == (sup(256, 384, c, c, 3, 3, 1, 1, 1, mode) if by_rule else 0), (h, w, c)
        # never for the other convolution kinds of the encoder / refinement block
        assert sup(h, w, c, c, 3, 3, 2, 1, 1, mode) == 0                          # stride 2
        assert sup(h, w, c, c, 1, 1, 1, 0, 0, mode) == 0                          # 1x1
        assert sup(h, w, c, c, 5, 1, 1, 2, 0, mode) == 0 and sup(h, w, c, c, 1, 5, 1, 0, 2, mode) == 0
        assert sup(h, w, c, c, 3, 3, 1, 0, 0, mode) == 0 and sup(h, w, c, c, 3, 3, 1, 1, 0, mode) == 0      # not "same" padding
    assert seen[0] > 0
    # the maps the issue names: 68 x 132 is admitted by the coverage rule, 34 x 66 and 17 x 33 are not; nothing at 120 x 200's maps
    assert parts(68, 132, 64, 3, 3, 1, 1, 1) == _patch_parts(68, 132)
    for h, w in ((34, 66), (17, 33), (60, 100), (30, 50), (15, 25)):
        assert all(sup(h, w, c, c, 3, 3, 1, 1, 1, 0) == 0 for c in (64, 96, 128))
    # bad geometry: 0, not an error exit
    assert sup(0, 32, 64, 64, 3, 3, 1, 1, 1, 0) == 0 and sup(64, 96, 48, 64, 3, 3, 1, 1, 1, 0) == 0       # cin % 32
    assert sup(64, 96, 64, 64, 3, 3, 1, 1, 1, 2) == 0 and sup(64, 96, 64, 30, 3, 3, 1, 1, 1, 0) == 0      # mode, cout % 4
    assert sup(64, 96, 64, 32, 3, 3, 1, 1, 1, 0) == 0                            # the 32-wide head tile has no on-load twin


def test_norm_on_load_entry_points_reject_bad_arguments_without_a_launch():
    lib = _abi.load()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    conv = lib.um_conv2d_norm_fwd
    ok_geo = (1, 64, 96, 64, 64, 3, 3, 1, 1, 1, 0, 10, 0, None)                 # batch .. stream
    assert conv(None, fake, 1, fake, None, fake, None, *ok_geo) == -1            # no input
    assert conv(fake, None, 1, fake, None, fake, None, *ok_geo) == -1            # no statistics
    assert b'statistics' in lib.um_last_error_string()
    assert conv(odd, fake, 1, fake, None, fake, None, *ok_geo) == -1             # input not 16-byte aligned
    assert conv(fake, fake, 1, None, None, fake, None, *ok_geo) == -1            # no weights
    assert conv(fake, fake, 1, fake, None, None, None, *ok_geo) == -1            # no output
    assert conv(fake, fake, 1, fake, odd, fake, None, *ok_geo) == -1 and b'aligned' in lib.um_last_error_string()
    assert conv(fake, fake, 1, fake, None, fake, None, 1, 64, 96, 48, 64, 3, 3, 1, 1, 1, 0, 10, 0, None) == -1       # cin % 32
    # geometries the patch kernel does not serve: an error, not another kernel and not a wrong answer
    for geo in ((64, 96, 64, 64, 3, 3, 2, 1, 1), (64, 96, 64, 64, 1, 1, 1, 0, 0), (64, 96, 64, 64, 5, 1, 1, 2, 0),
                (34, 66, 64, 64, 3, 3, 1, 1, 1), (8, 12, 64, 64, 3, 3, 1, 1, 1)):
        assert lib.um_conv2d_norm_supported(*geo, 0) == 0
        assert conv(fake, fake, 1, fake, None, fake, None, 1, *geo, 0, 10, 0, None) == -2, geo
        assert b'um_conv2d_norm_supported' in lib.um_last_error_string()
    fin = lib.um_nhwc_stats_finalize
    assert fin(None, 4, fake, 1, 512, 64, 1e-5, None) == -1 and fin(fake, 0, fake, 1, 512, 64, 1e-5, None) == -1
    assert fin(fake, 4, None, 1, 512, 64, 1e-5, None) == -1 and fin(fake, 4, fake, 0, 512, 64, 1e-5, None) == -1
    assert fin(fake, 4, fake, 1, 512, 60, 1e-5, None) == -1 and fin(fake, 4, fake, 1, 512, 264, 1e-5, None) == -1
    assert b'um_nhwc_stats_finalize' in lib.um_last_error_string()
    assert _abi.CENSUS['conv_patch_norm'] == 14 and lib.um_census_count(14) >= 0 and lib.um_census_count(15) == -1
