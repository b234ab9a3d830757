"""Shared helpers of tests/test_dispatch_boundaries_cpu.py and tests/test_dispatch_boundaries_gpu.py: every hot entry point picks a
kernel instantiation, or a code path inside one kernel, by a host-side rule on the call's geometry; the two files put one case on
each side of every such rule.  Here: seeded inputs, the exported plan / split / part-count functions wrapped so that a threshold
that depends on the CU count is SEARCHED for (never written down for 256 CUs), Python restatements of the rules that are plain
arithmetic on the arguments (each cites its line), the fp64 references that more than one row shares, and the record line every row
prints (profiles/dispatch_boundaries.txt is the collected output).  Nothing here needs a GPU."""
import ctypes
import functools
import math

import torch

from oracle import hotpath as hp

C = 128
UM_ERR_BAD_ARG, UM_ERR_UNSUPPORTED = -1, -4


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tok(fmap):
    return fmap.flatten(2).transpose(1, 2).contiguous()


def err(a, b):
    d = (a.double().cpu() - b.double().cpu()).abs()
    return d.max().item(), d.mean().item()


def record(row, geometry, side, variant, worst, gate, cus):
    """One line per row and case: what profiles/dispatch_boundaries.txt holds."""
    print(f'DISPATCH | {row} | {geometry} | {side} | {variant} | worst {worst:.3e} | gate {gate:.3e} | CUs {cus}')


# ------------------------------------------------------------------ rules that are plain arithmetic on the arguments
TAB_BYTES = 8192                  # window_attn.hip:144


def attn_uses_token_table(win_h, win_w):
    """window_attn.hip:231 -- ``use_tab = ntiles * TK * 4 <= TAB_BYTES`` with TK = 32 keys per tile: windows of up to 2048 tokens."""
    return (win_h * win_w + 31) // 32 * 32 * 4 <= TAB_BYTES


PIXEL_GRID_CAP = 256 * 16         # local_pixel.h:107: workgroups of 4 waves, one pixel per wave and trip


def pixel_grid_trips(pixels):
    """local_pixel.h:105 (pixel_grid_blocks) and the ``pid += gridDim.x * 4`` loops behind it: trips of the busiest wave."""
    blocks = min((pixels + 3) // 4, PIXEL_GRID_CAP)
    return (pixels + 4 * blocks - 1) // (4 * blocks)


def depth_uses_box_kernel(candidates):
    """local_ops.hip:812, 841 and depth_multi.hip:679, 746 -- lane = candidate while the candidates fit one wave."""
    return candidates <= 64


LOCAL_MAX_TAPS = 16 * 8           # local_pixel.h:7 (LOCAL_MAX_ROUNDS 8), checked at local_ops.hip:673, :792, :806, :831
K4_MAX_TAPS = 81                  # local_ops.hip:100, checked at :691, :774


def conv_tile_width(cout):
    """conv.hip:1191 -- the widest output tile (units of 32 columns) that does not waste more than a third of its columns."""
    return 4 if (cout % 128 == 0 or cout > 192) else 3 if cout % 96 == 0 else 2 if (cout <= 64 or cout % 64 == 0) else 4


def conv_kind(hi, wi, cout, kh, kw, stride, ph, pw):
    """conv.hip:1189-1209 (conv_pick) restated -> ('patch' | 'rows' | 'generic', NT of the launch).  Used to say what a row of the
    table MEANS to reach; what it reached is read from the launch census and um_conv_stats_parts."""
    ho, wo = (hi + 2 * ph - kh) // stride + 1, (wi + 2 * pw - kw) // stride + 1
    nt = conv_tile_width(cout)
    same = stride == 1 and ho == hi and wo == wi and ho * wo >= 256
    rows3, rows5 = same and kw == 3 and pw == 1, same and kw == 5 and pw == 2 and nt == 4
    tiled = (ho + 7) // 8 * 8 * ((wo + 31) // 32 * 32)
    if rows3 and kh == 3 and ph == 1 and 4 * ho * wo >= 3 * tiled:
        return 'patch', (1 if cout <= 32 else nt)
    return ('rows' if rows3 or rows5 else 'generic'), nt


def conv_parts(kind, ho, wo):
    """conv.hip:1243-1250 -- statistics parts per image: two per 8 x 32 tile of the patch kernel, else one per 128 pixels."""
    return 2 * ((ho + 7) // 8) * ((wo + 31) // 32) if kind == 'patch' else (ho * wo + 127) // 128


NORM_CHUNK_ROWS, NORM_PARTS_IN_REGISTERS = 256, 1024      # nhwc_ops.hip:15, :86-87 (32 lanes x NB = 32 parts held in registers)


# ------------------------------------------------------------------ the exported plan functions
def attn_plan(lib, streams, h, w, win_h, win_w):
    """um_window_attn_plan -> (tiles served whole, tiles served key-split, parts per split tile)."""
    f, r, p = (ctypes.c_int() for _ in range(3))
    rc = lib.um_window_attn_plan(streams, h, w, win_h, win_w, ctypes.byref(f), ctypes.byref(r), ctypes.byref(p))
    assert rc == 0, rc
    return f.value, r.value, p.value


def attn_parts(lib, streams, h, w, win_h, win_w):
    full, split, parts = attn_plan(lib, streams, h, w, win_h, win_w)
    assert (full == 0) != (split == 0)                 # window_attn.hip:1119-1130: a launch is all whole tiles or all key-split
    nbytes = lib.um_window_attn_ksplit_workspace_bytes(streams, h, w, win_h, win_w)
    assert (nbytes > 0) == (split > 0), (nbytes, split)
    return parts if split else 1


def attn_unsplit_streams(lib, h, w, win_h, win_w, limit=64):
    """The smallest stream count at which the launch is not key-split (window_attn.hip:1094-1129)."""
    for s in range(1, limit + 1):
        if attn_parts(lib, s, h, w, win_h, win_w) == 1:
            return s
    raise AssertionError(f'no stream count up to {limit} leaves {win_h}x{win_w} windows on a {h}x{w} map unsplit')


# one window geometry whose tile count moves in steps of four: 16 x 32 = 512 tokens = 4 query tiles of 128, 16 key tiles (enough for
# 4 parts of >= 4 tiles each); a map of k windows stacked has 4 k tiles.  No geometry reaches EVERY tile count: a window that may
# split at all has >= 8 key tiles = more than 224 tokens = at least 2 query tiles, so its launches count tiles in multiples of >= 2
# and "one past" a step is the next reachable count.
STEP_WINDOW = (16, 32)


def attn_split_steps(lib, max_windows=1024):
    """[(k, k + 1, parts at k, parts at k + 1)]: the numbers k of stacked STEP_WINDOW windows (one stream) after which the launch's
    part count changes -- the ``total * 2 * split <= 2 * CUs`` steps of window_attn.hip:1100, searched for on this device."""
    wh, ww = STEP_WINDOW
    parts = [attn_parts(lib, 1, wh * k, ww, wh, ww) for k in range(1, max_windows + 2)]
    return [(k, k + 1, parts[k - 1], parts[k]) for k in range(1, max_windows + 1) if parts[k - 1] != parts[k]]


def ffn_split(lib, m, hidden):
    """The hidden split um_ffn_ws_fwd takes when it is given the workspace um_ffn_split_workspace_bytes asks for (ffn.hip:978-996):
    the byte count is counters (256-byte aligned) + tiles x split slots of 64 x 256 floats."""
    nbytes = lib.um_ffn_split_workspace_bytes(m, hidden)
    if nbytes == 0:
        return 1
    tiles = (m + 127) // 128
    head = (tiles * 4 + 255) // 256 * 256
    split, rem = divmod(nbytes - head, tiles * 64 * 256 * 4)
    assert rem == 0 and split in (2, 4), (m, hidden, nbytes)
    return split


def ffn_split_steps(lib, hidden, max_tiles=4096):
    """[(m, m + 1, split at m, split at m + 1)] with m a multiple of 128: the token counts after which the split changes
    (``tiles * 2 * split <= CUs``, ffn.hip:983), searched for on this device."""
    out = []
    for t in range(1, max_tiles + 1):
        a, b = ffn_split(lib, 128 * t, hidden), ffn_split(lib, 128 * t + 1, hidden)
        if a != b:
            out.append((128 * t, 128 * t + 1, a, b))
    return out


def ffn_split_rule(m, hidden, cus):
    """ffn.hip:978-985 restated, for the slice-count conditions (hidden / 32 slices divisible by 2 x split, >= 4 per part)."""
    tiles, nslice, split = (m + 127) // 128, hidden // 32, 1
    while split < 4 and tiles * 2 * split <= cus and nslice % (2 * split) == 0 and nslice // (2 * split) >= 4:
        split *= 2
    return split


def attn_split_rule(total, key_tiles, cus):
    """window_attn.hip:1094-1129 restated: parts per tile of a launch of ``total`` query tiles with ``key_tiles`` key tiles each."""
    split = 1
    if total <= 2 * cus:
        while split < 4 and total * 2 * split <= 2 * cus and key_tiles >= 4 * 2 * split:
            split *= 2
    return split


# ------------------------------------------------------------------ fp64 references shared by several rows
def layer_norm_params(seed_w, seed_b, c=C):
    norm = torch.nn.LayerNorm(c)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.1 * rnd(seed_w, c))
        norm.bias.copy_(0.1 * rnd(seed_b, c))
    return norm


def merged_layer_reference(x, xt, wq, wk, wv, wm, norm, streams, h, w, geom, rot, residual):
    """fp64 composition of the merged attention layer (um_window_attn_merge_fwd / um_window_attn_qproj_merge_fwd): attention of stream
    s against the keys / values of stream (s + rot) mod S -- an explicit rotation of the key / value streams -- through the oracle's
    window attention, then merge Linear + LayerNorm (+ residual).  x, xt: fp32 ``[S * L, C]`` source tokens of q and of k | v."""
    c = x.shape[1]
    l = h * w
    q64 = (x.double() @ wq.double().t()).view(streams, l, c)
    kv_src = xt.double().view(streams, l, c).roll(-rot, 0)                  # stream s reads stream (s + rot) mod S
    k64, v64 = kv_src @ wk.double().t(), kv_src @ wv.double().t()
    att = hp.window_attention(q64, k64, v64, h, w, *geom)
    want = torch.nn.functional.layer_norm(att.reshape(streams * l, c) @ wm.double().t(), (c,), norm.weight.double().cpu(),
                                          norm.bias.double().cpu(), norm.eps)
    if residual:
        want = want + x.double()
    return want


def ffn_reference(x, y, w1, w2, norm):
    """fp64 ``x + LayerNorm(W2 . gelu(W1 . [x | y]))`` (the reference of test_fused_ffn_kernel)."""
    hid = torch.nn.functional.gelu(torch.cat([x, y], 1).double() @ w1.double().t())
    return x.double() + torch.nn.functional.layer_norm(hid @ w2.double().t(), (128,), norm.weight.double().cpu(),
                                                       norm.bias.double().cpu(), norm.eps)


def make_local_features(b, h, w):
    """f0, f1 ``[B, C, h, w]`` fp32 with real correspondences (the inputs of test_local_kernels_random_shapes)."""
    f0, f1 = rnd(500 + h, b, C, h, w), rnd(501 + w, b, C, h, w)
    return f0, 0.5 * f0.roll((1, 1), (2, 3)) + 0.5 * f1


# the caches below are bounded: they hold the few small maps that neighbouring tests share (8 MB a map at 128 x 128), never the
# one-off large cases, which call the builders directly
local_features = functools.lru_cache(maxsize=4)(make_local_features)


@functools.lru_cache(maxsize=4)
def sweep_features(b, h, w):
    """The plane sweep's inputs of test_plane_sweep_box_and_gather_paths: ``f1 = 0.6 roll(f0) + 0.4 noise``."""
    f0, f1 = rnd(1500, b, C, h, w), rnd(1501, b, C, h, w)
    return f0, 0.6 * f0.roll((0, 2), (2, 3)) + 0.4 * f1


def sweep_camera(b, h, w, move=(0.12, -0.03, 0.02)):
    """(K [B, 3, 3], pose [B, 4, 4], packed cam [B, 30] = K^-1 | R | t | K) of a sideways move, fx = 0.9 w."""
    fx = 0.9 * w
    k = torch.tensor([[fx, 0, w / 2], [0, fx, h / 2], [0, 0, 1.0]])[None].repeat(b, 1, 1)
    pose = torch.eye(4)[None].repeat(b, 1, 1)
    pose[:, :3, 3] = torch.tensor(move)
    cam = torch.cat([torch.inverse(k).flatten(1), pose[:, :3, :3].flatten(1), pose[:, :3, 3], k.flatten(1)], 1).contiguous()
    return k, pose, cam


def sweep_candidates(nd):
    return torch.linspace(1 / 10.0, 1 / 0.5, nd)


@functools.lru_cache(maxsize=32)                       # results of one plane ``[B, 1, h, w]`` each
def sweep_reference(b, h, w, nd, argmax, dtype=torch.float64):
    f0, f1 = sweep_features(b, h, w)
    k, pose, _ = sweep_camera(b, h, w)
    return hp.depth_corr_softmax(f0.to(dtype), f1.to(dtype), k.to(dtype), pose.to(dtype), sweep_candidates(nd).to(dtype), argmax)


SWEEP_COUNTS = (1, 16, 17, 64, 65, 128)        # degenerate | a full 16-slot round | one past it | box kernel's last | gather's first | limit
SWEEP_SMALL = (1, 13, 19)                      # 247 pixels: no multiple of a workgroup's 4 waves


def prop_local_reference(q, k, value, radius):
    """attention.py:217-253 on given q, k maps ``[B, C, h, w]`` (fp64): out-of-image neighbours have key 0 (logit 0) and value 0 and
    take part in the softmax."""
    c = q.shape[1]
    logits, vals = [], []
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ks, _ = hp._shifted(k, dy, dx)
            vs, _ = hp._shifted(value, dy, dx)
            logits.append((q * ks).sum(1) / math.sqrt(c))
            vals.append(vs)
    prob = torch.softmax(torch.stack(logits, 1), dim=1)
    return (prob.unsqueeze(2) * torch.stack(vals, 1)).sum(1)
