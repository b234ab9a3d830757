"""Every HipOps kernel wrapper under the memory-contract harness (tests/memory_guard.py): no write outside a buffer (W), inputs
stay as they were (I), the result does not depend on what fresh memory holds (U) nor on the bytes around the inputs (R), and two
runs agree bit for bit.  No tolerance anywhere: raw bytes are compared.  One table of cases keyed by method name; the completeness
test fails when a public method has neither a case nor a reason in EXCLUDED.  Shapes are the smallest that reach each dispatch
path with a ragged tail (taken from the fp64 tests of the same kernels where those have lists)."""
import inspect
import os

import pytest
import torch

from tests import memory_guard as mg
from tests import test_memory_guard_cpu as standins
from unimatch_amd import UniMatch, _abi
from unimatch_amd.ops import HipOps
from unimatch_amd.synth import CONFIGS, synth_camera, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
C = 128
BOTH = ('exact', 'fast')           # ops that take self.mode run in both operand precisions

# Regions of a RETURNED buffer that are unspecified by contract and masked out of U: {method: (citation, mask function)}.  An entry
# needs the sentence that makes the region unspecified and a composition test (below) that contains the consumer and passes unmasked.
DONT_CARE = {}
# Ops that are not bit-reproducible run to run: {method: cause (which atomic, which arrival order)}.  None is known.
NOT_REPRODUCIBLE = {}

EXCLUDED = {
    'graph_scope': 'scope: a context manager over the workspace registry, no kernel',
    'part_scope': 'scope: a context manager over the workspace registry, no kernel',
    'workspace_scope': 'scope: returns the current (token, lane), pure host',
    'workspace_entries': 'cache management: a read-only view of the registry for tests',
    'release_cached_planes': 'cache management: drops registry entries',
    'invalidate_weights': 'cache management: clears the weight-plane cache and the registry',
    'cached_planes_buffer': 'cache management: planes_buffer through the registry (exercised by the NhwcUpdateBlock composition)',
    'kv4_slices': 'pure host helper: offsets into blocked planes',
    'conv2d_norm_supported': '*_supported query: a pure function of the geometry',
    'conv2d_entry_supported': '*_supported query: a pure function of the geometry',
}

CASES = {}


def case(method, name, modes=('exact',)):
    def deco(f):
        CASES.setdefault(method, []).append((name, modes, f))
        return f
    return deco


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def T(g, seed, *shape, scale=1.0):
    return g.place(rnd(seed, *shape, scale=scale))


def layer_norm(g, seed):
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(seed, C))
        norm.bias.copy_(0.1 * rnd(seed + 1, C))
    return g.place_module(norm)


# ====================================================================== linear family
MS = (1, 127, 129, 257)


@case('weight_planes', 'one [128,128]; cat of [128,128] + [256,128]', BOTH)
def _(ops, g):
    a = ops.weight_planes((T(g, 1, 128, 128, scale=0.1),))
    b = ops.weight_planes((T(g, 2, 128, 128, scale=0.1), T(g, 3, 256, 128, scale=0.1)))
    return a, b


@case('kv4_weight_planes', 'four [128,128]', BOTH)
def _(ops, g):
    return ops.kv4_weight_planes(tuple(T(g, 10 + i, 128, 128, scale=0.09) for i in range(4)))


@case('linear_planes', 'm in 1,127,129,257: n 128 / K-concat + gelu n 256 / planes input', BOTH)
def _(ops, g):
    w, w256, w2 = T(g, 20, 128, 128, scale=0.1), T(g, 21, 256, 256, scale=0.1), T(g, 22, 384, 128, scale=0.1)
    out = []
    for m in MS:
        a, a1 = T(g, 23 + m, m, 128, scale=2.0), T(g, 24 + m, m, 128, scale=2.0)
        p, _, n = ops.linear_planes(a, (w,))
        out += [p, ops.linear_planes(a, (w256,), a1=a1, gelu=True)[0], ops.linear_planes(p, (w2,), a_planes_k=n)[0]]
    return out


@case('linear_ln', 'm in 1,127,129,257: plain / residual / planes input', BOTH)
def _(ops, g):
    w, w2, norm = T(g, 30, 128, 128, scale=0.1), T(g, 31, 128, 256, scale=0.1), layer_norm(g, 32)
    out = []
    for m in MS:
        a, res = T(g, 34 + m, m, 128, scale=2.0), T(g, 35 + m, m, 128)
        hid, _, n = ops.linear_planes(a, (T(g, 36, 256, 128, scale=0.1),))
        out += [ops.linear_ln(a, (w,), norm), ops.linear_ln(a, (w,), norm, residual=res), ops.linear_ln(hid, (w2,), norm, residual=res, a_planes_k=n)]
    return out


@case('linear_bias', 'm in 1,127,129,257: fp32 / planes out / planes in', BOTH)
def _(ops, g):
    w, bias = T(g, 40, 128, 128, scale=0.1), T(g, 41, 128)
    out = []
    for m in MS:
        a = T(g, 42 + m, m, 128, scale=2.0)
        p = ops.linear_bias(a, w, bias, out_mul=0.5, bias_mul=0.5, planes=True)
        out += [ops.linear_bias(a, w, bias), p, ops.linear_bias(p, w, bias, planes=True, a_planes_k=128)]
    return out


def _ffn_weights(g, hidden):
    return T(g, 50 + hidden, hidden, 256, scale=0.08), T(g, 51 + hidden, 128, hidden, scale=0.06), layer_norm(g, 52)


def _smallest_split_m(ops, hidden):
    for m in range(1, 4097):
        if ops.lib.um_ffn_split_workspace_bytes(m, hidden) > 0:
            return m
    raise AssertionError('no m <= 4096 takes the hidden-split launch')


@case('ffn_ln', 'm in 1,127,129,257 x hidden 64,1024', BOTH)
def _(ops, g):
    out = []
    for hidden in (64, 1024):
        w1, w2, norm = _ffn_weights(g, hidden)
        out += [ops.ffn_ln(T(g, 53 + m, m, 128, scale=1.5), T(g, 54 + m, m, 128, scale=1.5), w1, w2, norm) for m in MS]
    return out


@case('ffn_ln', 'the smallest m with a split workspace, hidden 1024, twice (the workspace is handed out again)', BOTH)
def _(ops, g):
    m = _smallest_split_m(ops, 1024)
    w1, w2, norm = _ffn_weights(g, 1024)
    x, y = T(g, 55, m, 128, scale=1.5), T(g, 56, m, 128, scale=1.5)
    return ops.ffn_ln(x, y, w1, w2, norm), ops.ffn_ln(x, y, w1, w2, norm), m


@case('ffn_ln_kv', 'm in 1,127,129,257 and the smallest split m x hidden 64,1024', BOTH)
def _(ops, g):
    ws = tuple(T(g, 60 + i, 128, 128, scale=0.09) for i in range(4))
    out = []
    for hidden in (64, 1024):
        w1, w2, norm = _ffn_weights(g, hidden)
        for m in MS + (_smallest_split_m(ops, 1024),):
            out += list(ops.ffn_ln_kv(T(g, 64 + m, m, 128, scale=1.5), T(g, 65 + m, m, 128, scale=1.5), w1, w2, norm, ws))
    return out


@case('kv4_planes', 'm in 1,127,129,257', BOTH)
def _(ops, g):
    ws = tuple(T(g, 70 + i, 128, 128, scale=0.09) for i in range(4))
    return [ops.kv4_planes(T(g, 74 + m, m, 128, scale=1.7), ws) for m in MS]


# ====================================================================== window attention
# (streams, h, w, win_h, win_w, shift_h, shift_w, kv_rotate) from test_query_projection_prologue_matches_q_planes: shifted 2-D windows
# of 15 tokens with rotation 2; shifted 1-D windows; one 240-token window (ragged last query tile and key tile) with rotation 1
WINDOWS = ((4, 6, 10, 3, 5, 1, 2, 2), (2, 9, 40, 1, 10, 0, 5, 1), (2, 12, 20, 12, 20, 0, 0, 1))
KSPLIT_CANDIDATES = ((1, 32, 48, 32, 48, 0, 0, 0), (2, 32, 48, 16, 24, 8, 12, 1), (2, 40, 56, 20, 28, 10, 14, 1))


def _ksplit_geometry(ops):
    for geo in WINDOWS + KSPLIT_CANDIDATES:
        if ops.lib.um_window_attn_ksplit_workspace_bytes(*geo[:5]) > 0:
            return geo
    raise AssertionError('no geometry takes the key-split launch')


def _attn_operands(ops, g, geo):
    s_, h, w = geo[:3]
    m = s_ * h * w
    x, xt = T(g, 900 + h, m, C, scale=1.5), T(g, 901 + w, m, C, scale=1.5)
    wq, wk, wv, wm = (T(g, 902 + i, C, C, scale=0.09) for i in range(4))
    qp, _, _ = ops.linear_planes(x, (wq,))
    kv, _, n2 = ops.linear_planes(xt, (wk, wv))
    return x, m, wq, wm, layer_norm(g, 906), (qp, m, C, 0), (kv, m, n2, 0), (kv, m, n2, C)


@case('window_attention', 'three ragged geometries', BOTH)
def _(ops, g):
    out = []
    for s_, h, w, wh, ww, sh, sw, _ in WINDOWS:
        q, k, v = (T(g, 910 + i, s_, h * w, C) for i in range(3))
        out.append(ops.window_attention(q, k, v, h, w, wh, ww, sh, sw))
    return out


@case('window_attention_planes', 'three ragged geometries, kv_rotate', BOTH)
def _(ops, g):
    out = []
    for geo in WINDOWS:
        x, m, wq, wm, norm, q, k, v = _attn_operands(ops, g, geo)
        out.append(ops.window_attention_planes(q, k, v, geo[0], *geo[1:7], kv_rotate=geo[7]))
    return out


@case('window_attention_merge', 'three ragged geometries, with and without residual', BOTH)
def _(ops, g):
    out = []
    for i, geo in enumerate(WINDOWS):
        x, m, wq, wm, norm, q, k, v = _attn_operands(ops, g, geo)
        out.append(ops.window_attention_merge(q, k, v, geo[0], *geo[1:8], wm, norm, x if i != 1 else None))
    return out


@case('window_attention_qproj_merge', 'three ragged geometries, with and without residual', BOTH)
def _(ops, g):
    out = []
    for i, geo in enumerate(WINDOWS):
        x, m, wq, wm, norm, q, k, v = _attn_operands(ops, g, geo)
        out.append(ops.window_attention_qproj_merge(x, wq, k, v, geo[0], *geo[1:8], wm, norm, x if i != 1 else None))
    return out


@case('window_attention_qproj_merge', 'a key-split geometry, twice (the workspace is handed out again)', BOTH)
def _(ops, g):
    geo = _ksplit_geometry(ops)
    x, m, wq, wm, norm, q, k, v = _attn_operands(ops, g, geo)
    call = lambda: ops.window_attention_qproj_merge(x, wq, k, v, geo[0], *geo[1:8], wm, norm, x)
    return call(), call(), geo


# ====================================================================== global matching
# 7x9 at b = 1 and b = 36 and a single row (gsv3_kernel, the small launch); 24x40 at b = 36, the shape of
# test_global_matching_offset_renormalisation: 15 key tiles, >= 8 per CU, which gsv4_kernel needs (7x9 has one key tile at any batch)
GLOBAL_SHAPES = ((1, 7, 9), (36, 7, 9), (2, 1, 7), (36, 24, 40))


@case('global_corr_softmax_flow', '7x9 at b=1 and b=36, 1x7, 24x40 at b=36; with and without bidir', BOTH)
def _(ops, g):
    out = []
    for b, h, w in GLOBAL_SHAPES:
        f0, f1 = T(g, 100 + b, b, h * w, C), T(g, 101 + b, b, h * w, C)
        out += [ops.global_corr_softmax_flow(f0, f1, h, w), ops.global_corr_softmax_flow(f0, f1, h, w, bidir=True)]
    return out


@case('global_corr_softmax_stereo', '7x9 at b=1 and b=36, 1x7, 24x40 at b=36', BOTH)
def _(ops, g):
    return [ops.global_corr_softmax_stereo(T(g, 110 + b, b, h * w, C), T(g, 111 + b, b, h * w, C), h, w) for b, h, w in GLOBAL_SHAPES]


@case('prop_global', '7x9 at b=1 and b=36, 1x7, 24x40 at b=36; 2 and 1 value channels', BOTH)
def _(ops, g):
    out = []
    for b, h, w in GLOBAL_SHAPES:
        q, k = T(g, 120 + b, b, h * w, C), T(g, 121 + b, b, h * w, C)
        out += [ops.prop_global(q, k, T(g, 122 + v, b, v, h, w, scale=3.0), h, w) for v in (2, 1)]
    return out


@case('prop_global_projected', '7x9 at b=1 and b=36, 1x7, 24x40 at b=36; 2 and 1 value channels', BOTH)
def _(ops, g):
    torch.manual_seed(11)
    qp, kp = g.place_module(torch.nn.Linear(C, C)), g.place_module(torch.nn.Linear(C, C))
    out = []
    for b, h, w in GLOBAL_SHAPES:
        tokens = T(g, 130 + b, b, h * w, C)
        out += [ops.prop_global_projected(tokens, qp, kp, T(g, 131 + v, b, v, h, w, scale=3.0), h, w) for v in (2, 1)]
    return out


# ====================================================================== local kernels
LOCAL_SHAPES = ((2, 9, 11), (2, 16, 24))          # 9x11: VALU kernels only; 16x24: whole 8 x 4 tiles, the matrix-core kernels at radius 4


def _matrix_core_serves_16x24(ops):
    assert ops.lib.um_local_corr_with_flow_feat_supported(16, 24, C, 4) and not ops.lib.um_local_corr_with_flow_feat_supported(9, 11, C, 4)


def _features(g, seed, b, h, w):
    return T(g, seed, b, h * w, C), T(g, seed + 1, b, h * w, C)


@case('local_corr_softmax', '9x11 and 16x24 (matrix-core path where supported), radius 4 and 2, one_d')
def _(ops, g):
    _matrix_core_serves_16x24(ops)
    out = []
    for b, h, w in LOCAL_SHAPES:
        f0, f1 = _features(g, 200 + h, b, h, w)
        out += [ops.local_corr_softmax(f0, f1, h, w, 4), ops.local_corr_softmax(f0, f1, h, w, 2), ops.local_corr_softmax(f0, f1, h, w, 4, one_d=True)]
    return out


@case('local_corr_with_flow', '9x11 and 16x24, radius 4, dilation 1 and 2, matrix-core and VALU kernels')
def _(ops, g):
    _matrix_core_serves_16x24(ops)
    out = []
    for b, h, w in LOCAL_SHAPES:
        f0, f1 = _features(g, 210 + h, b, h, w)
        flow = T(g, 212 + h, b, 2, h, w, scale=3.0)
        out += [ops.local_corr_with_flow(f0, f1, flow, h, w, 4), ops.local_corr_with_flow(f0, f1, flow, h, w, 4, dilation=2)]
        ops.k4_mfma = False
        out.append(ops.local_corr_with_flow(f0, f1, flow, h, w, 4))
        ops.k4_mfma = True
    return out


@case('local_corr_with_flow_planes', '9x11 and 16x24 into zeroed planes of ld 96, matrix-core and VALU kernels')
def _(ops, g):
    _matrix_core_serves_16x24(ops)
    out = []
    for b, h, w in LOCAL_SHAPES:
        f0, f1 = _features(g, 220 + h, b, h, w)
        flow = T(g, 222 + h, b, 2, h, w, scale=3.0)
        for mfma in (True, False):
            ops.k4_mfma = mfma
            dest = ops.planes_buffer(b * h * w, 96)
            ops.local_corr_with_flow_planes(f0, f1, flow, h, w, 4, dest, 96)
            out.append(dest)
        ops.k4_mfma = True
    return out


@case('prop_local', '9x11 and 16x24, radius 1 and 2, 2 and 1 value channels')
def _(ops, g):
    out = []
    for b, h, w in LOCAL_SHAPES:
        q, k = _features(g, 230 + h, b, h, w)
        out += [ops.prop_local(q, k, T(g, 232, b, 2, h, w, scale=3.0), h, w, 1), ops.prop_local(q, k, T(g, 233, b, 1, h, w, scale=3.0), h, w, 2)]
    return out


def _cam(b, h, w, t):
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    pose[:, :3, 3] = torch.tensor(t)
    return torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous()


DEPTH_BOX = 160               # csrc/local_ops.hip: a pixel whose candidates' corners span more rows than this takes the per-pixel gather


def _box_positions(cam, cand, h, w):
    """Per pixel, the size of the bounding box of the candidates' corners as depth_corr_softmax_box_kernel computes it."""
    cm = cam[0].double()
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    r = cm[0:9].view(3, 3) @ torch.stack([xs.flatten(), ys.flatten(), torch.ones(h * w, dtype=torch.float64)])
    q = cm[9:18].view(3, 3) @ r                                                        # [3, L]
    pts = q[:, :, None] / cand.double()[None, None, :] + cm[18:21].view(3, 1, 1)        # [3, L, D]
    uvz = torch.einsum('ij,jld->ild', cm[21:30].view(3, 3), pts)
    z = uvz[2].clamp(min=1e-3)
    x0 = torch.floor(uvz[0] / z).clamp(-1, w - 1)
    y0 = torch.floor(uvz[1] / z).clamp(-1, h - 1)
    return (x0.amax(1) + 1 - x0.amin(1) + 1) * (y0.amax(1) + 1 - y0.amin(1) + 1)


@case('depth_corr_softmax', '9x11 and 16x24: box path (64 candidates), long diagonal (per-pixel fallback, reached at 16x24), gather kernel (80 candidates), arg-max')
def _(ops, g):
    out = []
    for b, h, w in LOCAL_SHAPES:
        f0, f1 = _features(g, 240 + h, b, h, w)
        for t, nd, argmax in (((0.12, -0.01, 0.0), 64, False), ((0.45, 0.40, 0.0), 64, False), ((0.12, -0.03, 0.02), 80, False), ((0.10, 0.02, 0.01), 64, True)):
            cand, cam = torch.linspace(1 / 10.0, 1 / 0.5, nd), _cam(b, h, w, t)
            npos = _box_positions(cam, cand, h, w)
            if t[1] == 0.40 and h == 16:          # the long diagonal at 16x24: pixels on both sides of the table size, well away from it
                assert (npos > DEPTH_BOX + 20).any() and (npos < DEPTH_BOX - 20).any(), (npos.min(), npos.max())
            elif nd <= 64 and t[1] != 0.40:       # (9x11 cannot exceed the table: at most 12 x 10 positions)
                assert (npos < DEPTH_BOX - 20).all(), npos.max()
            out.append(ops.depth_corr_softmax(f0, f1, h, w, g.place(cam), g.place(cand), from_argmax=argmax))
    return out


# ====================================================================== convolutions and norms
def _planes_of(ops, g, seed, b, c, h, w, scale=1.5):
    """Operand planes (and the fp32 NHWC form) of a placed NCHW map: um_nchw_to_nhwc, itself under the guard."""
    return ops.nchw_to_nhwc(T(g, seed, b, c, h, w, scale=scale), want_planes=True, want_f32=True)


def _conv_w(g, seed, cout, cin, kh, kw):
    return T(g, seed, cout, cin, kh, kw, scale=(2.0 / (cin * kh * kw)) ** 0.5)


@case('nchw_to_nhwc', '9x11 c 64, 37x29 c 96, 16x32 c 128: planes and fp32, planes only, fp32 only')
def _(ops, g):
    out = []
    for b, c, h, w in ((2, 64, 9, 11), (1, 96, 37, 29), (2, 128, 16, 32)):
        x = T(g, 300 + c, b, c, h, w)
        out += [ops.nchw_to_nhwc(x, True, True), ops.nchw_to_nhwc(x, True, False), ops.nchw_to_nhwc(x, False, True)]
    return out


@case('conv2d_nhwc', 'generic 9x11, patch 16x32, odd 37x29 at stride 2; c 64/96/128; stats; relu + bias; 1x1 with image_addend')
def _(ops, g):
    out = []
    #        b, cin, cout, h,  w,  k, stride, pad, bias, relu, stats
    for i, (b, cin, cout, h, w, k, stride, pad, bias, relu, stats) in enumerate((
            (2, 64, 64, 9, 11, 3, 1, 1, False, False, False), (2, 96, 96, 16, 32, 3, 1, 1, True, True, True),
            (1, 64, 96, 37, 29, 3, 2, 1, False, False, True), (1, 128, 128, 9, 11, 3, 1, 1, True, True, False),
            (2, 128, 128, 16, 32, 3, 1, 1, False, False, True), (1, 64, 96, 37, 29, 1, 2, 0, True, False, True))):
        planes, _ = _planes_of(ops, g, 310 + i, b, cin, h, w)
        y, ho, wo = ops.conv2d_nhwc((planes, b, h, w, cin), _conv_w(g, 320 + i, cout, cin, k, k), T(g, 330 + i, cout) if bias else None, stride,
                                    (pad, pad), relu, stats)
        out += [y, ho, wo, ops.last_conv_stats[0] if stats else None]
    for i, (b, c, h, w) in enumerate(((2, 128, 9, 11), (2, 128, 16, 32), (1, 64, 37, 29))):
        planes, _ = _planes_of(ops, g, 340 + i, b, c, h, w)
        out.append(ops.conv2d_nhwc((planes, b, h, w, c), _conv_w(g, 343 + i, c, c, 1, 1), T(g, 346 + i, c), 1, (0, 0), image_addend=T(g, 349 + i, h * w, c))[0])
    return out


NORMED_CANDIDATES = ((64, 16, 32), (96, 16, 32), (128, 16, 32), (64, 22, 60), (96, 30, 31), (128, 24, 32))


@case('conv2d_nhwc_normed', 'the supported ones of: 16x32 at c 64/96/128, ragged 22x60, 30x31, 24x32; with stats')
def _(ops, g):
    out, ran = [], 0
    for i, (c, h, w) in enumerate(NORMED_CANDIDATES):
        wt = _conv_w(g, 360 + i, c, c, 3, 3)
        if not ops.conv2d_norm_supported(h, w, c, wt):
            continue
        ran += 1
        planes, _ = _planes_of(ops, g, 370 + i, 2, c, h, w)
        t, _, _ = ops.conv2d_nhwc((planes, 2, h, w, c), _conv_w(g, 380 + i, c, c, 3, 3), None, 1, (1, 1), stats=True)
        u, _, _ = ops.conv2d_nhwc_normed(t, ops.last_conv_stats, (2, h, w, c), wt, stats=True)
        out += [u, ops.last_conv_stats[0]]
    assert ran, 'um_conv2d_norm_supported admits none of the candidate geometries'
    return out


ENTRY_CANDIDATES = ((64, 96, 22, 60), (96, 128, 17, 33), (64, 96, 31, 45), (96, 128, 16, 32), (64, 96, 37, 29))


@case('conv2d_entry', 'the supported ones of: 22x60, 17x33, 31x45, 16x32, 37x29 (odd at stride 2); c 64->96 and 96->128')
def _(ops, g):
    out, ran = [], 0
    for i, (cin, cout, h, w) in enumerate(ENTRY_CANDIDATES):
        w1, wp = _conv_w(g, 400 + i, cout, cin, 3, 3), _conv_w(g, 410 + i, cout, cin, 1, 1)
        if not ops.conv2d_entry_supported(h, w, cin, w1, wp):
            continue
        ran += 1
        planes, _ = _planes_of(ops, g, 420 + i, 2, cin, h, w)
        u, _, _ = ops.conv2d_nhwc((planes, 2, h, w, cin), _conv_w(g, 430 + i, cin, cin, 3, 3), None, 1, (1, 1), stats=True)
        shortcut, _ = _planes_of(ops, g, 440 + i, 2, cin, h, w)
        t, d, ho, wo, (st_t, _), (st_d, _) = ops.conv2d_entry(u, ops.last_conv_stats, shortcut, (2, h, w, cin), w1, wp, T(g, 450 + i, cout))
        out += [t, d, ho, wo, st_t, st_d]
    assert ran, 'um_conv2d_entry_supported admits none of the candidate geometries'
    return out


@case('conv_weight_planes', '[96,64,3,3]')
def _(ops, g):
    return ops.conv_weight_planes(_conv_w(g, 460, 96, 64, 3, 3))


@case('conv_weight_planes_from', '[128,64,3,3] and [4,256,3,3]')
def _(ops, g):
    return ops.conv_weight_planes_from(_conv_w(g, 461, 128, 64, 3, 3)), ops.conv_weight_planes_from(_conv_w(g, 462, 4, 256, 3, 3))


@case('conv_weight_padded', '[256,83,1,1] to 96 input channels')
def _(ops, g):
    return ops.conv_weight_padded(_conv_w(g, 463, 256, 83, 1, 1), 96)


@case('planes_buffer', 'rows 7, ld 96')
def _(ops, g):
    return ops.planes_buffer(7, 96)


@case('conv_ex', '9x11 (generic kernel) and 16x32 (patch kernel): column slice in, fp32 and planes out at column offsets, tanh')
def _(ops, g):
    out = []
    for b, h, w in ((2, 9, 11), (2, 16, 32)):
        rows, cin, cout = b * h * w, 64, 128
        src = ops.planes_buffer(rows, 96)
        ops.nhwc_gate(0, T(g, 470 + h, rows, 96), src, 96, 0, rows, 96)
        dst = ops.planes_buffer(rows, 256)
        f32 = torch.zeros((rows, 160), dtype=torch.float32, device=DEV)
        wb = (ops.conv_weight_planes_from(T(g, 471, cout, cin, 3, 3, scale=0.05)), T(g, 472, cout))
        ops.conv_ex((src, 96, 32, cin), (b, h, w), wb, (3, 3), 1, (1, 1), 3, out=(f32, 160, 32), outp=(dst, 256, 128))
        out += [src, dst, f32]
    return out


def _mask_gate_rows(raw):
    """conv_gru's case returns (G, ZR, H) triples: of each ZR row [256] the gate-1 launch writes the z half."""
    raw = list(raw)
    for i in range(1, len(raw), 3):
        zr = raw[i].clone().view(-1, 256 * 4)
        zr[:, 128 * 4:] = 0
        raw[i] = zr.view(-1)
    return tuple(raw)


DONT_CARE['conv_gru'] = ('DESIGN.md, "Memory contract": "gate 1 of um_conv2d_gru_fwd / um_conv2d_gru_add_fwd writes `channels` columns (z) of every z_out '
                         'row; with z_out_ld = 2 * channels, as NhwcUpdateBlock.ZR has it, columns channels .. 2 * channels - 1 are never written and '
                         'never read (gate 2 reads z at z_ld)" (consumer: test_update_block_composition, unmasked)', _mask_gate_rows)


@case('conv_gru', '9x11 and 16x32: gate 1 and gate 2 (1x5 and 5x1), plain (state updated in place) and with addend + hidden_out')
def _(ops, g):
    out = []
    for b, h, w in ((2, 9, 11), (1, 16, 32)):
        rows, geo = b * h * w, (b, h, w)
        for ks, pad in (((1, 5), (0, 2)), ((5, 1), (2, 0))):
            G = ops.planes_buffer(rows, 512)
            ops.nhwc_gate(0, T(g, 480 + h, rows, 384), G, 512, 0, rows, 384)
            H = g.place(torch.tanh(rnd(481 + h, rows, 128)), inout=True)
            ZR = torch.empty((rows, 256), dtype=torch.float32, device=DEV)
            zr = (ops.conv_weight_planes_from(T(g, 482, 256, 384, *ks, scale=0.03)), T(g, 483, 256))
            q = (ops.conv_weight_planes_from(T(g, 484, 128, 384, *ks, scale=0.03)), T(g, 485, 128))
            ops.conv_gru(1, (G, 512, 0, 384), geo, zr, ks, pad, H, (G, 512, 384), z_out=ZR)
            ops.conv_gru(2, (G, 512, 128, 384), geo, q, ks, pad, H, (G, 512, 0), z=ZR)
            out += [G, ZR, H]
            # hoisted form: only the changing columns, the rest enters as the epilogue's addend; the state is read, the new one goes to H2
            G2 = ops.planes_buffer(rows, 512)
            ops.nhwc_gate(0, T(g, 486 + h, rows, 384), G2, 512, 0, rows, 384)
            net0 = g.place(torch.tanh(rnd(487 + h, rows, 128)))
            ZR2, H2 = torch.empty((rows, 256), dtype=torch.float32, device=DEV), torch.empty((rows, 128), dtype=torch.float32, device=DEV)
            zrv = (ops.conv_weight_planes_from(T(g, 488, 256, 128, *ks, scale=0.03)), None)
            qv = (ops.conv_weight_planes_from(T(g, 489, 128, 256, *ks, scale=0.03)), None)
            ops.conv_gru(1, (G2, 512, 256, 128), geo, zrv, ks, pad, net0, (G2, 512, 384), z_out=ZR2, addend=T(g, 490, rows, 256))
            ops.conv_gru(2, (G2, 512, 256, 256), geo, qv, ks, pad, net0, (G2, 512, 128), z=ZR2, addend=T(g, 491, rows, 128), hidden_out=H2)
            out += [G2, ZR2, H2]
    return out


@case('conv7', '9x11 and 16x32 at stride 1: 2 and 1 image channels -> planes, fp32 out; 37x29 with 3 channels at stride 2')
def _(ops, g):
    out = []
    for b, h, w in ((2, 9, 11), (2, 16, 32)):
        rows = b * h * w
        for fd in (2, 1):
            F1 = ops.planes_buffer(rows, 128)
            ops.conv7(T(g, 500 + fd, b, fd, h, w, scale=2.0), T(g, 501 + fd, 128, fd, 7, 7, scale=0.1), T(g, 503, 128), 1, 1, outp=(F1, 128, 0))
            out.append(F1)
        f32 = torch.zeros((rows, 128), dtype=torch.float32, device=DEV)
        ops.conv7(T(g, 504, b, 2, h, w, scale=2.0), T(g, 505, 128, 2, 7, 7, scale=0.1), None, 1, 0, out=(f32, 128, 0))
        out.append(f32)
    half = torch.zeros((2 * 19 * 15, 64), dtype=torch.float32, device=DEV)                # stride 2 (the stem's packing) through this wrapper
    ops.conv7(T(g, 506, 2, 3, 37, 29, scale=2.0), T(g, 507, 64, 3, 7, 7, scale=0.1), T(g, 508, 64), 2, 1, out=(half, 64, 0))
    out.append(half)
    return out


@case('stem_conv', '37x29 b 2 and 16x32 b 1, raw and with input normalisation, with statistics; a pair of 2 + 1 images')
def _(ops, g):
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    wt = T(g, 510, 64, 3, 7, 7, scale=0.12)
    out = []
    for b, h, w in ((2, 37, 29), (1, 16, 32)):
        img = g.place(rnd(511 + h, b, 3, h, w).abs() * 120.0)
        for nm in (None, norm):
            out += [ops.stem_conv(img, wt, nm)[0], ops.last_conv_stats[0]]
        out.append(ops.stem_conv(img, wt, None, stats=False)[0])
    pair = (g.place(rnd(513, 2, 3, 37, 29).abs() * 120.0), g.place(rnd(514, 1, 3, 37, 29).abs() * 120.0))
    out += [ops.stem_conv(pair, wt, norm)[0], ops.last_conv_stats[0]]
    return out


@case('instance_norm', 'NCHW 36x29 c 64 b 2 (261 float4 per plane), 5x4 c 128 (less than a wave): relu, shortcut')
def _(ops, g):
    out = []
    for shape in ((2, 64, 36, 29), (3, 128, 5, 4)):            # the kernel takes planes of a multiple of 4 pixels
        x, sc = T(g, 520, *shape, scale=3.0), T(g, 521, *shape)
        out += [ops.instance_norm(x, relu=False), ops.instance_norm(x, relu=True, shortcut=sc)]
    return out


@case('nhwc_norm', '9x11 c 64, 37x29 c 96, 16x32 c 128: plain, fp32 shortcut, shortcut planes, no normalisation, conv statistics, shortcut statistics')
def _(ops, g):
    out = []
    for b, c, h, w in ((2, 64, 9, 11), (1, 96, 37, 29), (2, 128, 16, 32)):
        rows = b * h * w
        x, sc = T(g, 530 + c, rows, c, scale=2.0), T(g, 531 + c, rows, c)
        scp, _ = _planes_of(ops, g, 532 + c, b, c, h, w)
        out += [ops.nhwc_norm(x, b, h * w, want_planes=True, want_f32=True), ops.nhwc_norm(x, b, h * w, shortcut=sc, want_f32=True),
                ops.nhwc_norm(x, b, h * w, shortcut_planes=scp), ops.nhwc_norm(x, b, h * w, normalize=False, relu=False)]
        planes, _ = _planes_of(ops, g, 533 + c, b, c, h, w)
        y, _, _ = ops.conv2d_nhwc((planes, b, h, w, c), _conv_w(g, 534 + c, c, c, 3, 3), None, 1, (1, 1), stats=True)
        ystats = ops.last_conv_stats
        d, _, _ = ops.conv2d_nhwc((planes, b, h, w, c), _conv_w(g, 535 + c, c, c, 1, 1), T(g, 536 + c, c), 1, (0, 0), stats=True)
        out += [ops.nhwc_norm(y, b, h * w, conv_stats=ystats, want_f32=True),
                ops.nhwc_norm(y, b, h * w, conv_stats=ystats, shortcut=d, shortcut_stats=ops.last_conv_stats, want_f32=True)]
    return out


@case('nhwc_gate', '9x11 and 16x32: column scatter (96 and a ragged 2 columns at an even offset), r * h, state update')
def _(ops, g):
    out = []
    for b, h, w in ((2, 9, 11), (2, 16, 32)):
        rows = b * h * w
        zr, hb, q = g.place(torch.sigmoid(rnd(540, rows, 256))), g.place(rnd(541, rows, 128), inout=True), g.place(torch.tanh(rnd(542, rows, 128)))
        buf = ops.planes_buffer(rows, 512)
        ops.nhwc_gate(0, T(g, 543, rows, 96), buf, 512, 128, rows, 96)
        ops.nhwc_gate(1, None, buf, 512, 384, rows, 128, zr=zr, hbuf=hb)
        ops.nhwc_gate(2, q, buf, 512, 0, rows, 128, zr=zr, hbuf=hb)
        ops.nhwc_gate(0, T(g, 544, rows, 2), buf, 512, 382, rows, 2)
        out += [buf, hb]
    return out


@case('nhwc_concat_planes', '9x11 and 16x32, b 2: 2 and 1 flow channels + 128 tokens')
def _(ops, g):
    out = []
    for b, h, w in ((2, 9, 11), (2, 16, 32)):
        out += [ops.nhwc_concat_planes(T(g, 550 + v, b, v, h, w, scale=3.0), T(g, 552, b * h * w, C)) for v in (2, 1)]
    return out


@case('nhwc_planes_from', '99 rows: 2 + 81 channels padded to 96; 128 channels as they are')
def _(ops, g):
    return ops.nhwc_planes_from([T(g, 560, 99, 2), T(g, 561, 99, 81)]), ops.nhwc_planes_from([T(g, 562, 99, 128)])


# ====================================================================== upsampling, warping
@case('convex_upsample', '5x7 b 2: (factor, channels, depth) = (8,2,F) (4,2,F) (8,1,T) (4,1,F); NCHW and NHWC masks; out=')
def _(ops, g):
    out = []
    b, h, w = 2, 5, 7
    for factor, v, is_depth in ((8, 2, False), (4, 2, False), (8, 1, True), (4, 1, False)):
        flow, mask = T(g, 600 + factor, b, v, h, w, scale=5.0), rnd(601 + factor, b, 9 * factor * factor, h, w, scale=2.0)
        nhwc = g.place(mask.permute(0, 2, 3, 1).reshape(b * h * w, -1))
        dest = torch.empty((b, v, factor * h, factor * w), dtype=torch.float32, device=DEV)
        out += [ops.convex_upsample(flow, g.place(mask), factor, is_depth), ops.convex_upsample(flow, nhwc, factor, is_depth, mask_nhwc=True),
                ops.convex_upsample(flow, nhwc, factor, is_depth, mask_nhwc=True, out=dest)]
    return out


@case('flow_warp', '9x11 and 13x17, b 2: sub-pixel, integer and far-outside offsets')
def _(ops, g):
    out = []
    for h, w in ((9, 11), (13, 17)):
        flow = rnd(610, 2, 2, h, w, scale=4.0)
        flow[0, :, :3] = torch.tensor([2.0, -1.0]).view(2, 1, 1)
        flow[1, :, -2:] = 40.0
        out.append(ops.flow_warp(T(g, 611, 2, h * w, C), g.place(flow), h, w))
    return out


@case('flow_upsample2x', '9x11 b 2 with 2 channels, 37x53 b 1 with 1 channel')
def _(ops, g):
    return ops.flow_upsample2x(T(g, 620, 2, 2, 9, 11, scale=3.0), 2.0), ops.flow_upsample2x(T(g, 621, 1, 1, 37, 53, scale=3.0), 1.0)


# ====================================================================== video, pre / post, colour maps, metrics, geometry
ODD = (2, 37, 53)
PARTIALS = ((2, 37, 53), (1, 63, 65), (2, 17, 241))          # 4095 and 4097 pixels: either side of the 4096-pixel partial


@case('fwd_bwd_occlusion', '37x53 b 2, 5x3 b 1')
def _(ops, g):
    out = []
    for b, h, w in (ODD, (1, 5, 3)):
        fwd = rnd(700, b, 2, h, w, scale=3.0)
        out.append(ops.fwd_bwd_occlusion(g.place(fwd), g.place(-fwd + 0.4 * rnd(701, b, 2, h, w))))
    return out


@case('flow_to_rgb', '37x53 b 2, 63x65 (4095 pixels), 17x241 b 2 (4097 pixels)')
def _(ops, g):
    return [ops.flow_to_rgb(T(g, 710 + h, b, 2, h, w, scale=4.0)) for b, h, w in PARTIALS]


@case('scalar_to_rgb', '37x53 b 2, 63x65, 17x241 b 2: both normalisations, inverse, statistics')
def _(ops, g):
    lut = g.place(torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(720), dtype=torch.uint8))
    out = []
    for b, h, w in PARTIALS:
        x = g.place(rnd(721 + h, b, h, w).abs() + 0.1)
        out += [ops.scalar_to_rgb(x, lut), ops.scalar_to_rgb(x, lut, inverse=True, norm='min_p95_256', return_stats=True),
                ops.scalar_to_rgb(x, lut, norm='min_p95_256'), ops.scalar_to_rgb(x, lut, inverse=True, return_stats=True)]
    return out


@case('flow_chain', '3 pairs of 37x53: dense at stride 1 and 3 with and without occlusion; 257 sparse points with a start mask')
def _(ops, g):
    p, h, w = 3, 37, 53
    flow, occ = T(g, 730, p, 2, h, w, scale=2.0), g.place((rnd(731, p, h, w) > 1.0).float())
    pts = torch.rand(257, 2, generator=torch.Generator().manual_seed(732)) * torch.tensor([w + 4.0, h + 4.0]) - 2.0
    pts[5] = float('nan')
    pts[6] = torch.tensor([w - 1.0, h - 1.0])
    alive = g.place(torch.arange(257) % 7 != 0)
    return [ops.flow_chain(flow), ops.flow_chain(flow, occ, stride=3), ops.flow_chain(flow, occ), ops.flow_chain(flow, occ, points=g.place(pts), alive=alive),
            ops.flow_chain(flow, points=g.place(pts))]


@case('image_prepare', '37x53 b 2: pad and resize, fp32 and uint8 images, normalisation, hflip, transpose, out=')
def _(ops, g):
    b, h, w = ODD
    f32 = g.place(rnd(740, b, 3, h, w).abs() * 90.0)
    u8 = g.place(torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(741), dtype=torch.uint8))
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    out = []
    for images in (f32, u8):
        for hflip in (False, True):
            out += [ops.image_prepare(images, (40, 56), 'pad', (2, 1), hflip=hflip), ops.image_prepare(images, (48, 64), 'resize', mean=mean, std=std, hflip=hflip),
                    ops.image_prepare(images, (56, 40), 'pad', (1, 2), transpose=True, mean=mean, std=std, hflip=hflip),
                    ops.image_prepare(images, (24, 72), 'resize', transpose=True, hflip=hflip)]
    dest = torch.empty((b, 3, 40, 56), dtype=torch.float32, device=DEV)
    out.append(ops.image_prepare(u8, (40, 56), 'pad', (3, 3), out=dest))
    return out


@case('pred_restore', 'to 37x53 b 2: crop and resize of flow, disparity and depth, hflip, transpose, out=')
def _(ops, g):
    b, h, w = ODD
    out = []
    for kind, c in (('flow', 2), ('disparity', 1), ('depth', 1)):
        padded, resized, padded_t = T(g, 750 + c, b, c, 40, 56, scale=3.0), T(g, 751 + c, b, c, 48, 64, scale=3.0), T(g, 752 + c, b, c, 56, 40, scale=3.0)
        for hflip in (False, True):
            out += [ops.pred_restore(padded, (h, w), 'pad', (2, 1), kind, hflip=hflip), ops.pred_restore(resized, (h, w), 'resize', kind=kind, hflip=hflip),
                    ops.pred_restore(padded_t, (h, w), 'pad', (1, 2), kind, transpose=True, hflip=hflip),
                    ops.pred_restore(resized, (h, w), 'resize', kind=kind, transpose=True, hflip=hflip)]
    dest = torch.empty((b, 2, h, w), dtype=torch.float32, device=DEV)
    out.append(ops.pred_restore(T(g, 753, b, 2, 40, 56), (h, w), 'pad', (3, 3), 'flow', out=dest))
    return out


@case('flow_metrics', '37x53 b 2 and 63x65 / 17x241: plain; with valid, noc_valid and a crop of a padded prediction')
def _(ops, g):
    out = []
    for b, h, w in PARTIALS:
        gt = rnd(760, b, 2, h, w, scale=12.0)
        pred_padded = T(g, 761, b, 2, h + 5, w + 3, scale=12.0)
        valid, noc = g.place((rnd(762, b, h, w) > -1.0).float()), g.place((rnd(763, b, h, w) > 0.0).float())
        out += [ops.flow_metrics(g.place(gt + rnd(764, b, 2, h, w)), g.place(gt)), ops.flow_metrics(pred_padded, g.place(gt), valid, noc, crop=(2, 1)),
                ops.flow_metrics(pred_padded, g.place(gt), valid, crop=(5, 3))]
    return out


@case('disp_metrics', '37x53 b 2 and 63x65 / 17x241: plain; max_disp with a crop of a padded prediction')
def _(ops, g):
    out = []
    for b, h, w in PARTIALS:
        gt = g.place(rnd(770, b, h, w).abs() * 40.0 * (rnd(771, b, h, w) > -1.0))
        out += [ops.disp_metrics(T(g, 772, b, h, w, scale=30.0), gt), ops.disp_metrics(T(g, 773, b, h + 5, w + 3, scale=30.0), gt, max_disp=60.0, crop=(2, 1))]
    return out


@case('depth_metrics', '37x53 b 2 and 63x65 / 17x241: plain; valid, range and a crop of a padded prediction')
def _(ops, g):
    out = []
    for b, h, w in PARTIALS:
        gt = g.place(rnd(780, b, h, w).abs() * 4.0 + 0.2)
        valid = g.place((rnd(781, b, h, w) > -1.0).float())
        out += [ops.depth_metrics(g.place(rnd(782, b, h, w).abs() * 4.0 + 0.2), gt),
                ops.depth_metrics(g.place(rnd(783, b, h + 5, w + 3).abs() * 4.0 + 0.2), gt, valid, lo=0.5, hi=8.0, crop=(2, 1))]
    return out


def _camera(g, b, h, w, seed):
    k = torch.tensor([[0.9 * w, 0., (w - 1) / 2.], [0., 0.9 * w, (h - 1) / 2.], [0., 0., 1.]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    ang = 0.03 * torch.arange(1, b + 1)
    pose[:, 0, 0], pose[:, 0, 1], pose[:, 1, 0], pose[:, 1, 1] = torch.cos(ang), -torch.sin(ang), torch.sin(ang), torch.cos(ang)
    pose[:, :3, 3] = 0.05 * rnd(seed, b, 3) + torch.tensor([0.1, 0.0, 0.02])
    return g.place(k), g.place(pose)


@case('depth_cam', 'b 1, 2, 3: one-way and bidir')
def _(ops, g):
    out = []
    for b in (1, 2, 3):
        k, pose = _camera(g, b, 37, 53, 790)
        out += [ops.depth_cam(k, pose, 8.0), ops.depth_cam(k, pose, 1.0, bidir=True)]
    return out


@case('relative_pose_pairs', 'T = 2 and 5')
def _(ops, g):
    return [ops.relative_pose_pairs(_camera(g, t, 37, 53, 791)[1]) for t in (2, 5)]


@case('rigid_flow', '37x53 b 2, 5x3 b 1')
def _(ops, g):
    out = []
    for b, h, w in (ODD, (1, 5, 3)):
        k, pose = _camera(g, b, h, w, 792)
        out.append(ops.rigid_flow(g.place(1.0 / (rnd(793, b, 1, h, w).abs() * 3.0 + 0.5)), ops.depth_cam(k, pose, 1.0)))
    return out


@case('disp_consistency', '37x53 b 2, 64x97 b 1, 5x3')
def _(ops, g):
    out = []
    for b, h, w in (ODD, (1, 64, 97), (1, 5, 3)):
        dl = rnd(800, b, h, w).abs() * 6.0
        out.append(ops.disp_consistency(g.place(dl), g.place(dl + 0.5 * rnd(801, b, h, w))))
    return out


@case('depth_consistency', '37x53 b 2, 64x97 b 1, 5x3: mask only and with the two error maps; invalid depths')
def _(ops, g):
    out = []
    for b, h, w in (ODD, (1, 64, 97), (1, 5, 3)):
        k, pose = _camera(g, b, h, w, 810)
        cam = ops.depth_cam(k, pose, 1.0, bidir=True)
        ref, src = rnd(811, b, h, w).abs() * 0.2 + 2.0, rnd(812, b, h, w).abs() * 0.2 + 2.0
        ref[0, 0, 0], src[0, 1, 1], src[0, 2, 2] = 0.0, float('nan'), float('inf')
        ref, src = g.place(ref), g.place(src)
        out += [ops.depth_consistency(ref, src, cam[:b], cam[b:]), ops.depth_consistency(ref, src, cam[:b], cam[b:], return_errors=True)]
    return out


def _mask_points(raw):
    """points_pack returns buffers of M candidate rows of which the first N = count are written."""
    def one(xyz, rgb, count):
        n = int(count.view(torch.int32)[0])
        xyz = xyz.clone()
        xyz[12 * n:] = 0
        if rgb is not None:
            rgb = rgb.clone()
            rgb[3 * n:] = 0
        return xyz, rgb, count
    return tuple(one(*r) for r in raw)


DONT_CARE['points_pack'] = ('DESIGN.md, "Memory contract": "um_points_pack writes rows 0 .. N - 1 of xyz / rgb (N = count); rows N .. M - 1 are not '
                            'written and hold whatever the caller\'s buffer held" (consumer: test_point_cloud_composition, unmasked)', _mask_points)


@case('points_pack', '33x47 b 3 at stride 1 and 3: depth range, keep mask, colours; 5x3 without either')
def _(ops, g):
    b, h, w = 3, 33, 47
    k, pose = _camera(g, b, h, w, 820)
    cam = ops.depth_cam(k, pose, 1.0)
    depth = g.place(rnd(821, b, h, w).abs() * 2.0 + 0.2)
    keep = g.place((rnd(822, b, h, w) > -0.5).float())
    colors = g.place(torch.randint(0, 256, (b, h, w, 3), generator=torch.Generator().manual_seed(823), dtype=torch.uint8))
    k1, p1 = _camera(g, 1, 5, 3, 824)
    return (ops.points_pack(depth, cam, keep, colors, 0.3, 3.0, 1), ops.points_pack(depth, cam, keep, colors, 0.3, 3.0, 3), ops.points_pack(depth, cam, None, None, stride=3),
            ops.points_pack(g.place(rnd(825, 1, 5, 3).abs() + 0.2), ops.depth_cam(k1, p1, 1.0)))


# ====================================================================== the table, run
# Launch variants (unimatch_amd/_abi.CENSUS) that a case must reach: a change of a dispatch rule or of a *_supported predicate that drops
# a kernel from the contract fails here instead of passing quietly.  {(method, case index): counters that must be non-zero}
REACHES = {('local_corr_softmax', 0): ('k3_mfma', 'k3_valu'), ('local_corr_with_flow', 0): ('k4_mfma', 'k4_valu'),
           ('local_corr_with_flow_planes', 0): ('k4_mfma', 'k4_valu'), ('conv2d_nhwc', 0): ('conv_patch', 'conv_generic'),
           ('conv_ex', 0): ('conv_patch', 'conv_generic'), ('conv2d_nhwc_normed', 0): ('conv_patch_norm',), ('ffn_ln', 0): ('ffn_tile',),
           ('ffn_ln', 1): ('ffn_hsplit',), ('ffn_ln_kv', 0): ('ffn_hsplit',), ('window_attention_qproj_merge', 0): ('wattn_tile',),
           ('window_attention_qproj_merge', 1): ('wattn_ksplit',), ('global_corr_softmax_flow', 0): ('gsv3', 'gsv4'),
           ('global_corr_softmax_stereo', 0): ('gsv3',),        # (keys of one row, causal form: never gsv4)
           ('prop_global', 0): ('gsv3', 'gsv4'), ('prop_global_projected', 0): ('gsv3', 'gsv4')}

PARAMS = [(method, i, mode) for method in sorted(CASES) for i, (_, modes, _) in enumerate(CASES[method]) for mode in modes]


@pytest.mark.parametrize('method,index,mode', PARAMS, ids=[f'{m}-{i}-{p}' for m, i, p in PARAMS])
def test_op_memory_contract(method, index, mode):
    name, _, fn = CASES[method][index]
    mask = DONT_CARE[method][1] if method in DONT_CARE else None
    lib = _abi.load()
    lib.um_census_enable(1)
    try:
        first = mg.contract(fn, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps(mode), mask=mask)
        census = _abi.census(lib)
    finally:
        lib.um_census_enable(0)
    assert first is not None, name
    missed = [k for k in REACHES.get((method, index), ()) if census[k] == 0]
    assert not missed, f'{method}: "{name}" never launched {missed}: {census}'
    assert not mg.contract.last_passed_through, f'allocations on the device that the guard did not understand: {mg.contract.last_passed_through}'
    assert any(site.startswith('unimatch_amd') for site in mg.contract.last_sites), 'no allocation of the product went through the guard'


def test_every_public_method_has_a_case_or_a_reason():
    public = [n for n, f in inspect.getmembers(HipOps, predicate=inspect.isfunction) if not n.startswith('_')]
    assert len(public) > 60
    missing = [n for n in public if n not in CASES and n not in EXCLUDED]
    assert not missing, f'no memory-contract case (tests/test_memory_contract_gpu.py) and no reason in EXCLUDED: {missing}'
    stale = [n for n in list(CASES) + list(EXCLUDED) if n not in public]
    assert not stale, f'named in the table but not a public HipOps method: {stale}'
    assert not set(CASES) & set(EXCLUDED)
    assert all(len(reason) > 10 for reason in EXCLUDED.values())
    for method in sorted(CASES):
        takes_mode = 'self.mode' in inspect.getsource(getattr(HipOps, method))
        modes = {m for _, ms, _ in CASES[method] for m in ms}
        assert not takes_mode or modes == set(BOTH), f'{method} reads self.mode: its cases run in both precisions'
    assert all(m in CASES and cite for m, (cite, _) in DONT_CARE.items()) and all(NOT_REPRODUCIBLE.values())
    design = ' '.join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'DESIGN.md')).read().split())
    for method, (cite, _) in DONT_CARE.items():                      # the cited sentence stands where the entry says it does
        sentence = cite.split('": "', 1)[1].split('" (', 1)[0]
        assert len(sentence) > 40 and sentence in design, (method, sentence)


# ====================================================================== compositions: no region is "don't care" once a later kernel reads it
@pytest.mark.parametrize('iterations', [1, 3], ids=['plain', 'hoisted'])
@pytest.mark.parametrize('fd', [2, 1])
def test_update_block_composition(fd, iterations):
    """NhwcUpdateBlock through begin + two iterate calls at 12x20 (the cached plane buffers, every convolution of the block, both GRU
    forms): masks and deltas of both iterations, unmasked."""
    from unimatch_amd.refine import BasicUpdateBlock
    from unimatch_amd.refine_nhwc import NhwcUpdateBlock
    b, h, w = 2, 12, 20

    def run(ops, g):
        torch.manual_seed(5)
        block = g.place_module(BasicUpdateBlock(corr_channels=81, downsample_factor=4, flow_dim=fd))
        proj = g.place_module(torch.nn.Conv2d(128, 256, 1))
        upd = NhwcUpdateBlock(ops, block, proj)
        upd.begin(T(g, 101, b, h * w, 128), b, h, w, iterations=iterations)
        assert upd.hoist == (iterations > 1)
        ori0, ori1 = T(g, 102, b, h * w, 128), T(g, 103, b, h * w, 128)
        out = []
        for step in range(2):
            flow = rnd(104, b, fd, h, w, scale=2.0) + 0.25 * step
            disp = torch.cat([-flow, torch.zeros(flow.shape)], 1) if fd == 1 else flow
            out += list(upd.iterate(ori0, ori1, g.place(disp), g.place(flow), True))
        return out

    mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: HipOps('exact'))


def test_point_cloud_composition():
    """The consumers of um_points_pack's buffers -- geometry.back_project_points (reads count, slices the rows) and
    geometry.fuse_depth_sequence (relative poses, consistency masks, votes, then the packed cloud) -- on placed device tensors,
    unmasked: the cloud's size and every row of it must not depend on what the unwritten tail rows hold."""
    from unimatch_amd import geometry
    t, h, w = 3, 33, 47

    def fresh():
        geometry._hip_ops = None               # the module's own HipOps: a fresh one per run

    def run(_, g):
        k, poses = _camera(g, t, h, w, 830)
        depths = rnd(831, t, h, w).abs() * 0.05 + 2.0
        depths[1, 4:9, 5:20] *= 1.5            # an inconsistent patch, and invalid pixels
        depths[0, 0, 0], depths[2, 1, 1] = 0.0, float('nan')
        depths = g.place(depths)
        colors = g.place(torch.randint(0, 256, (t, h, w, 3), generator=torch.Generator().manual_seed(832), dtype=torch.uint8))
        keep = g.place((rnd(833, t, h, w) > -0.5).float())
        cloud = geometry.back_project_points(depths, k[:1], poses, keep, colors, 0.3, 3.0, 3)
        plain = geometry.back_project_points(depths, k, poses)
        fused = geometry.fuse_depth_sequence(depths, k[:1], poses, colors, px_thr=2.0, rel_thr=0.05, stride=1)
        assert 0 < cloud[0].shape[0] < plain[0].shape[0] and 0 < fused['xyz'].shape[0] < plain[0].shape[0]
        return cloud, plain, (fused['xyz'], fused['rgb'], fused['keep'])

    try:
        mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=fresh)
    finally:
        geometry._hip_ops = None
    assert any('ops.py' in site for site in mg.contract.last_sites)


@pytest.mark.parametrize('glue', [True, False], ids=['all_fused', 'no_glue'])
@pytest.mark.parametrize('scales', [1, 2])
def test_encoder_composition(scales, glue):
    """CNNEncoder at 37x51 (odd at every stride) on a pair batch of 2 + 1 raw images with the input normalisation folded in."""
    from unimatch_amd.encoder import CNNEncoder
    norm = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))

    def make_ops():
        ops = HipOps('exact')
        assert ops.fused_conv and ops.norm_on_load and ops.fused_entry and ops.fused_glue
        ops.fused_glue = glue
        return ops

    def run(ops, g):
        torch.manual_seed(7)
        enc = g.place_module(CNNEncoder(128, scales).eval())
        x = (g.place((rnd(5, 2, 3, 37, 51).abs() * 90.0).clamp(0, 255)), g.place((rnd(6, 1, 3, 37, 51).abs() * 90.0).clamp(0, 255)))
        with torch.no_grad():
            return [o.contiguous() for o in enc(x, ops, norm)]

    mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=make_ops)


SIZES = {'gmflow_s1': (64, 96), 'gmstereo_s1': (64, 96), 'gmdepth_s1': (96, 128), 'gmflow_s2_rr6': (128, 192), 'gmstereo_s2_rr3': (128, 192)}   # test_hip_parity_gpu.SIZES
_state = {}


def _fresh_model(name):
    ck, _ = CONFIGS[name]
    model = UniMatch(**ck).eval()
    if name not in _state:
        _state[name] = synth_state_dict({k: v.shape for k, v in model.state_dict().items()}, refine_gain=0.02)
    model.load_state_dict(_state[name])
    return model.to(DEV)


@pytest.mark.parametrize('name,batch', [(n, 1) for n in SIZES] + [('gmflow_s1', 3)], ids=lambda v: str(v))
def test_whole_forward(name, batch):
    """A whole forward of a fresh model per run: the prediction is bit-identical across the fills and the input red zones and every
    red zone of every allocation of the forward is intact.  No exemption of any kind."""
    fk = CONFIGS[name][1]
    hh, ww = SIZES[name]
    i0, i1 = synth_images(batch, hh, ww, seed=1000, kind='shift', normalized=(fk['task'] != 'flow'))

    def run(model, g):
        kw = dict(fk)
        if fk['task'] == 'depth':
            k, pose = synth_camera(batch, hh, ww)
            kw.update(intrinsics=g.place(k), pose=g.place(pose))
        with torch.no_grad():
            pred = model(g.place(i0), g.place(i1), **kw)['flow_preds'][0]
        assert torch.isfinite(pred).all()
        return pred

    mg.contract(run, lambda guard: (guard,), device=DEV, make_ops=lambda: _fresh_model(name))
    sites = {site for site in mg.contract.last_sites if site.startswith('unimatch_amd')}
    assert len(mg.contract.last_sites) > 100 and len(sites) > 20, (len(mg.contract.last_sites), sorted(sites))


# ====================================================================== the harness itself, once on the device
def test_a_correct_stand_in_passes_on_the_device():
    mg.contract(standins.standin_good(DEV), standins.make_standin_inputs(DEV), device=DEV)


@pytest.mark.parametrize('defect,prop,text', standins.DEFECTS, ids=[d[0].__name__ for d in standins.DEFECTS])
def test_each_defect_is_caught_on_the_device(defect, prop, text):
    """Plain torch on device tensors, no project kernel: synchronisation and the comparison work here too.  All damage stays inside
    blocks this test owns (a byte of a red zone, an element of a placed input)."""
    with pytest.raises(mg.ContractViolation) as exc:
        mg.contract(defect(DEV), standins.make_standin_inputs(DEV), device=DEV)
    assert exc.value.prop == prop, str(exc.value)
    assert not text or text in str(exc.value), str(exc.value)
