"""The convolution dispatcher's answers over a grid of layer descriptors (helper, no tests).

The queries are host code and never touch their operands, so the descriptors are filled directly with a dummy address and full-size shapes cost
nothing.  tests/test_conv_route_sweep.py compares the in-tree library with the digests scripts/record_conv_routes.py stored in
tests/golden/conv_routes.json: a change that moves ANY route, split factor, slab height or weight-gradient split of the grid fails on the CPU."""
import ctypes
import hashlib
import itertools

from simpledepthestimation_amd.hip import nn as NN

F32, BF16, F16 = 0, 1, 2                     # SDE_F32 / SDE_BF16 / SDE_F16
DTYPES = {"bf16": BF16, "fp16": F16, "fp32": F32}
QUERIES = ("sde_conv_fwd_variant", "sde_conv_fwd_tiles_m", "sde_conv_fwd_ws_bytes", "sde_conv_dgrad_bnbwd_rows", "sde_conv_dgrad_bnbwd_res_rows",
           "sde_conv_wgrad_variant", "sde_conv_wgrad_splits")
DUMMY = 0x10000                              # never dereferenced

# (B, H, W) of the stored source x0
MAPS = ((1, 13, 21), (2, 6, 20), (12, 6, 20), (12, 12, 40), (4, 24, 80), (12, 24, 80), (12, 48, 160), (1, 192, 640), (12, 96, 320), (12, 192, 640),
        (4, 384, 1280))
CINS = (3, 8, 16, 32, 40, 48, 64, 96, 128, 193, 256, 512, 1024, 2048)        # real channels; stored padded to the 16-byte group
COUTS = (1, 8, 16, 24, 32, 64, 72, 128, 256, 512)
# (k, stride, pad, reflect): "same" zero padding, the full correlation a data gradient runs (pad k - 1), reflection padding
GEOMS = tuple((k, s, k // 2, 0) for k in (1, 3, 5, 7) for s in (1, 2)) + tuple((k, 1, k - 1, 0) for k in (3, 5, 7)) + \
    tuple((k, s, min(1, k // 2), 1) for k in (1, 3, 5, 7) for s in (1, 2))
KEEP = {NN.SRC_PLAIN: 0.045, NN.SRC_UPCAT: 0.03, NN.SRC_ZEROINS: 0.03}       # share of the full product that is enumerated (deterministic thinning)

# every option moved alone: (name, key or None for sde_conv_set_halo_min_blocks, value)
OPTION_SETS = (("defaults", None, None), ("pgemm=0", NN.OPT_PGEMM, 0), ("pgemm_depth=4", NN.OPT_PGEMM_DEPTH, 4), ("pgemm_3x3=1", NN.OPT_PGEMM_3X3, 1),
               ("pgemm_tile=128064", NN.OPT_PGEMM_TILE, 128064), ("pgemm_tile=128128", NN.OPT_PGEMM_TILE, 128128), ("splitk=0", NN.OPT_SPLITK, 0),
               ("splitk=64", NN.OPT_SPLITK, 64), ("wgrad_blocks=1024", NN.OPT_WGRAD_BLOCKS, 1024), ("wgrad_halo=0", NN.OPT_WGRAD_HALO, 0),
               ("conv_small=0", NN.OPT_CONV_SMALL, 0), ("wgrad_dma=0", NN.OPT_WGRAD_DMA, 0), ("bnbwd_fuse=0", NN.OPT_BNBWD_FUSE, 0),
               ("cu_reserve=64", NN.OPT_CU_RESERVE, 64), ("pgemm_per_cu=2", NN.OPT_PGEMM_PER_CU, 2), ("halo_min_blocks=0", None, 0),
               ("halo_min_blocks=-1", None, -1))


def bind(lib):
    """Prototypes of what the sweep calls, on any handle of the library (hip.lib's own, or a second build loaded beside it)."""
    D, I = ctypes.POINTER(NN.ConvDesc), ctypes.c_int
    for name, args, res in (("sde_conv_fwd_variant", (D, I), I), ("sde_conv_fwd_tiles_m", (D, I), I), ("sde_conv_fwd_ws_bytes", (D, I), ctypes.c_size_t),
                            ("sde_conv_dgrad_bnbwd_rows", (D, I, I), I), ("sde_conv_dgrad_bnbwd_res_rows", (D, I, I), I),
                            ("sde_conv_wgrad_variant", (D, I, I), I), ("sde_conv_wgrad_splits", (D, I), I), ("sde_conv_set_option", (I, I), I),
                            ("sde_conv_set_halo_min_blocks", (I,), I), ("sde_last_error", (), ctypes.c_char_p)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = list(args), res
    return lib


def pad_to(c, v):
    return (c + v - 1) // v * v


def make_desc(dtype, mode, B, H0, W0, C0, C1, IH, IW, k, stride, pad, reflect):
    d = NN.ConvDesc()
    d.x0, d.x1 = DUMMY, (DUMMY if C1 else None)
    d.dtype, d.C0, d.C1, d.H0, d.W0, d.IH, d.IW = dtype, C0, C1, H0, W0, IH, IW
    d.src_mode, d.KH, d.KW, d.stride, d.pad, d.reflect = mode, k, k, stride, pad, reflect
    d.Bn, d.OH, d.OW = B, (IH + 2 * pad - k) // stride + 1, (IW + 2 * pad - k) // stride + 1
    return d


def _kept(i, share):
    return (i * 2654435761) % (1 << 32) < share * (1 << 32)       # Knuth's multiplicative hash of the position in the full product


def descriptors(dtype):
    """[(ConvDesc, Cout, ldy)] of one storage type, in a fixed order; every one is a descriptor fill_gather accepts."""
    V = 4 if dtype == F32 else 8
    out = []
    for mode in (NN.SRC_PLAIN, NN.SRC_UPCAT, NN.SRC_ZEROINS):
        for i, ((B, H, W), cin, cout, (k, s, pad, reflect)) in enumerate(itertools.product(MAPS, CINS, COUTS, GEOMS)):
            if not _kept(i, KEEP[mode]):
                continue
            C0, C1, IH, IW = pad_to(cin, V), 0, H, W
            if mode == NN.SRC_UPCAT:                   # nearest x2 upsample of x0, concatenated with a skip tensor of half the channels (every other one: none)
                IH, IW, C1 = 2 * H, 2 * W, (pad_to(cin // 2, V) if i % 2 else 0)
            elif mode == NN.SRC_ZEROINS:               # data gradient of a stride-2 layer: stride 1 over the zero-inserted source, odd or even extent
                IH, IW, s, reflect = 2 * H - (i % 2), 2 * W - (i % 2), 1, 0
                pad = k - 1 - k // 2
            if IH > 384 or min(IH, IW) + 2 * pad < k:
                continue
            out.append((make_desc(dtype, mode, B, H, W, C0, C1, IH, IW, k, s, pad, reflect), cout, pad_to(cout, V)))
    return out


def answers(lib, d, Cout, ldy):
    r = ctypes.byref(d)
    return (lib.sde_conv_fwd_variant(r, ldy), lib.sde_conv_fwd_tiles_m(r, ldy), lib.sde_conv_fwd_ws_bytes(r, ldy), lib.sde_conv_dgrad_bnbwd_rows(r, Cout, ldy),
            lib.sde_conv_dgrad_bnbwd_res_rows(r, Cout, ldy), lib.sde_conv_wgrad_variant(r, Cout, ldy), lib.sde_conv_wgrad_splits(r, Cout))


def _set(lib, key, value):
    return lib.sde_conv_set_halo_min_blocks(value) if key is None else lib.sde_conv_set_option(key, value)


def sweep(lib, descs, option_sets=OPTION_SETS):
    """{option set: [answers of every descriptor]}; each option is moved alone and put back."""
    out = {}
    for name, key, value in option_sets:
        old = None if value is None else _set(lib, key, value)
        assert old is None or old >= 0 or key is None, f"{name}: sde_conv_set_option refused"
        try:
            out[name] = [answers(lib, d, Cout, ldy) for d, Cout, ldy in descs]
        finally:
            if value is not None:
                _set(lib, key, old)
    return out


def digest(rows):
    return hashlib.sha256("\n".join(",".join(map(str, t)) for t in rows).encode()).hexdigest()


def digests(lib):
    """{option set: {dtype: sha256 over the answers in enumeration order}} and the defaults' answers per dtype."""
    out, defaults = {}, {}
    for dt, code in DTYPES.items():
        descs = descriptors(code)
        res = sweep(lib, descs)
        defaults[dt] = (descs, res["defaults"])
        for name, rows in res.items():
            out.setdefault(name, {})[dt] = digest(rows)
    return out, defaults


# What the grid has to exercise at the defaults, each on at least MIN_COVER descriptors.
MIN_COVER = 20
COVER = ("staged 64x64", "staged 128x32", "staged 128x16", "halo N 64", "halo N 32", "halo N 16", "chalo", "pgemm", "split 2", "split 3..7", "split 8",
         "bnbwd pgemm", "bnbwd halo", "wgrad halo", "wgrad dma", "wgrad staged", "wgrad first-layer rule")


def histogram(defaults):
    """How many descriptors of the grid take each kernel / rule at the defaults (the coverage condition reads this)."""
    h = dict.fromkeys(COVER, 0)
    h["descriptors"] = h["refused"] = 0
    for descs, rows in defaults.values():
        for (d, Cout, ldy), (variant, tiles_m, ws, rows_bn, rows_res, wkind, wsplits) in zip(descs, rows):
            M, Cin = d.Bn * d.OH * d.OW, d.C0 + d.C1
            h["descriptors"] += 1
            h["refused"] += wkind == 0
            fam = variant // 1000000
            for name, hit in (("staged 64x64", variant == 64064), ("staged 128x32", variant == 128032), ("staged 128x16", variant == 128016),
                              ("halo N 64", variant == 3128064), ("halo N 32", variant == 3128032), ("halo N 16", variant == 3128016),
                              ("chalo", fam == 5), ("pgemm", fam == 7)):
                h[name] += hit
            S = ws // (M * ldy * 4)
            h["split 2"] += S == 2
            h["split 3..7"] += 3 <= S <= 7
            h["split 8"] += S == 8
            h["bnbwd pgemm"] += rows_bn > 0 and fam == 7
            h["bnbwd halo"] += rows_bn > 0 and fam == 3
            for name, kind in (("wgrad halo", 1), ("wgrad dma", 2), ("wgrad staged", 3)):
                h[name] += wkind == kind
            bmg = 64 if Cout > 32 else 32 if Cout > 16 else 16
            wtiles = -(-Cout // bmg) * -(-(d.KH * d.KW * Cin) // 128)
            h["wgrad first-layer rule"] += wkind != 1 and Cin <= 16 and M >= 65536 and wtiles <= 8
    return h
