"""The case table of tests/test_conv_edges_gpu.py: every convolution form at a ragged last tile, a column tile that is mostly
past Cout, a split that does not divide the k-tiles, a pixel walk that ends inside a k-tile.  No torch, no GPU: the table and
the arithmetic of its claims, checked by tests/test_conv_edge_cases_cpu.py.

A case is (name, (B, Cin, H, W, Cout, k, stride), forms, claims).  `forms` is what the thresholds of launch_conv /
launch_wgrad_tiles predict for the product build -- the counters are the judge, on the GPU.  `claims` say what makes the
case an edge case, as tuples the CPU test recomputes from the shape:
  ("last_m", form, r)       the last M-tile of `form`'s tile holds r rows, 0 < r < BM
  ("valid_n", form, c)      the last column tile of `form` holds c valid columns, 0 < c < BN (the rest is padding or nothing)
  ("splits", n, counters)   launch_conv splits the nk k-tiles n ways (with / without arrival counters) and nk % n != 0
  ("whole", counters)       launch_conv does not split (with / without arrival counters)
  ("dgrad_splits", n, counters)  the same for the stride-1 data gradient (K = k k Cout, N = Cin)
  ("pix16", r)              M % 16 == r != 0: the weight gradient's last k-tile of 16 pixels holds r
  ("short_image",)          Ho Wo < 16: a weight-gradient k-tile spans images
  ("wgrad_splits", n)       the weight gradient's pixel splits with the whole scratch, n > 1
  ("last_r", form, r)       the last row tile of the weight-gradient tile `form` holds r of its BM rows of R
  ("odd",)                  Ho and Wo are odd
"""
from collections import namedtuple

Case = namedtuple("Case", "name shape forms claims")

BK = 16
# (BM, BN) of a forward / data-gradient form (the split forms run the 64 x 64 tile) and of a weight-gradient form (rows of R)
TILE = {"128x32": (128, 32), "128x128_2x2": (128, 128), "128x128_4x1": (128, 128), "64x128": (64, 128), "64x64": (64, 64),
        "split_vec": (64, 64), "split_scalar": (64, 64), "split_inkernel": (64, 64), "split_inkernel_stats": (64, 64)}
WGRAD_TILE = {"wgrad_128x128": (128, 128), "wgrad_128x32": (128, 32), "wgrad_128x64": (128, 64), "wgrad_64x64": (64, 64)}
BIG_TILES = ("128x128_2x2", "128x128_4x1", "64x128")
SPLITK_SCRATCH = 8 * 1024 * 1024  # floats: what the forms file hands over, and the train scratch's split-K piece


def cdiv(a, b):
    return (a + b - 1) // b


def npad32(n):
    return cdiv(n, 32) * 32


def out_dim(H, k, stride):
    return (H + 2 * ((k - 1) // 2) - k) // stride + 1


Geometry = namedtuple("Geometry", "Ho Wo M K R Npad nk")


def geometry(shape):
    """M = B Ho Wo output pixels, K = R = k k Cin, Npad = Cout padded to 32, nk = k-tiles of 16 of the forward contraction."""
    B, Cin, H, W, Cout, k, s = shape
    Ho, Wo = out_dim(H, k, s), out_dim(W, k, s)
    K = k * k * Cin
    return Geometry(Ho, Wo, B * Ho * Wo, K, K, npad32(Cout), cdiv(K, BK))


def conv_splits(M, Npad, nk, counters, scratch_floats=SPLITK_SCRATCH):
    """The split count of launch_conv's 64 x 64 branch (conv_mfma.h): fewer than 700 workgroups, at least 32 (with arrival
    counters) / 64 k-tiles, towards 1280 workgroups, 8 at the most, 8 k-tiles per split at the least, inside the scratch."""
    wgs = cdiv(M, 64) * cdiv(Npad, 64)
    if wgs >= 700 or nk < (32 if counters else 64):
        return 1
    sp = min(8, cdiv(1280, wgs), nk // 8)
    return sp if sp > 1 and sp * M * Npad <= scratch_floats else 1


def wgrad_splits(R, Cout, M, form):
    """wgrad_want_splits (wgrad_mfma.h) for the whole scratch: 1024 workgroups, 256 splits and nk / 4 at the most."""
    bm, bn = WGRAD_TILE[form]
    return max(1, min(1024 // (cdiv(R, bm) * cdiv(Cout, bn)), 256, cdiv(M, BK) // 4))


def _both(forms):
    return {"f32": forms, "bf16x3": forms}  # (shared, never changed)


# ---- frlw_conv2d_fwd with split-K scratch and no arrival counters ---------------------------------------------------------------
FWD = [
    # A: ragged last M-tile, odd Ho x Wo
    Case("A 128x128 2x2, last tile 2 rows", (2, 64, 255, 319, 128, 1, 1), _both({"128x128_2x2"}),
         [("last_m", "128x128_2x2", 2), ("odd",)]),
    Case("A 64x128 / 4x1, last tile 2 / 66 rows", (2, 64, 127, 159, 256, 3, 1), {"f32": {"64x128"}, "bf16x3": {"128x128_4x1"}},
         [("last_m", "64x128", 2), ("last_m", "128x128_4x1", 66), ("odd",)]),
    Case("A 64x64, last tile 43 rows", (3, 64, 31, 39, 64, 3, 1), _both({"64x64"}), [("last_m", "64x64", 43), ("odd",), ("whole", False)]),
    Case("A 128x32, last tile 43 rows", (3, 64, 31, 39, 32, 3, 1), _both({"128x32"}), [("last_m", "128x32", 43), ("odd",)]),
    Case("A stride 2 to 127 x 159", (4, 64, 254, 318, 128, 3, 2), {"f32": {"64x128"}, "bf16x3": {"128x128_4x1"}},
         [("last_m", "64x128", 4), ("last_m", "128x128_4x1", 4), ("odd",)]),
    # B: the last column tile mostly past Cout
    Case("B 128x128 2x2, Cout 132", (2, 64, 255, 319, 132, 1, 1), _both({"128x128_2x2"}),
         [("valid_n", "128x128_2x2", 4), ("last_m", "128x128_2x2", 2), ("odd",)]),
    Case("B 64x128 / 4x1, Cout 132", (2, 64, 127, 159, 132, 3, 1), {"f32": {"64x128"}, "bf16x3": {"128x128_4x1"}},
         [("valid_n", "64x128", 4), ("valid_n", "128x128_4x1", 4), ("last_m", "64x128", 2), ("odd",)]),
    Case("B 64x64, Cout 72", (1, 64, 33, 41, 72, 3, 1), _both({"64x64"}), [("valid_n", "64x64", 8), ("last_m", "64x64", 9), ("odd",)]),
    Case("B split, Cout 132", (2, 256, 8, 10, 132, 3, 1), _both({"split_vec"}), [("valid_n", "split_vec", 4), ("last_m", "split_vec", 32)]),
    # C: splits that do not divide the k-tiles
    Case("C 81 k-tiles over 8", (2, 144, 8, 10, 256, 3, 1), _both({"split_vec"}), [("splits", 8, False), ("last_m", "split_vec", 32)]),
    Case("C 81 k-tiles over 8, M 80", (1, 144, 8, 10, 256, 3, 1), _both({"split_vec"}), [("splits", 8, False), ("last_m", "split_vec", 16)]),
    Case("C 44 k-tiles, whole without counters", (2, 704, 8, 10, 256, 1, 1), _both({"64x64"}), [("whole", False), ("last_m", "64x64", 32)]),
    Case("C M 189 over 8", (3, 256, 7, 9, 256, 3, 1), _both({"split_vec"}), [("last_m", "split_vec", 61), ("odd",)]),
]

# ---- frlw_baseconv_train_fwd / _bwd with arrival counters and no operand cache: (forward forms, backward forms) ------------------
TRAIN = [
    Case("A train 128x128 2x2, last slab 2 rows", (2, 64, 255, 319, 128, 1, 1),
         _both(({"128x128_2x2"}, {"64x64", "wgrad_64x64", "wgrad_group_sum"})), [("last_m", "128x128_2x2", 2), ("pix16", 2), ("odd",)]),
    Case("A train 64x128 / 4x1, last slab 2 / 66 rows", (2, 64, 127, 159, 256, 3, 1),
         {"f32": ({"64x128"}, {"split_inkernel", "wgrad_128x64"}), "bf16x3": ({"128x128_4x1"}, {"split_vec", "wgrad_128x64"})},
         [("last_m", "64x128", 2), ("last_m", "128x128_4x1", 66), ("pix16", 2), ("odd",)]),
    # 36 k-tiles: with the arrival counters this shape splits 4 ways -- the unsplit 64 x 64 tile with statistics is the next case
    Case("A train 64x64 shape, split 4 with counters, last slab 43 rows", (3, 64, 31, 39, 64, 3, 1),
         {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x64"})},
         [("last_m", "split_inkernel_stats", 43), ("pix16", 11), ("odd",)]),
    Case("A train 64x64 unsplit, last slab 43 rows", (3, 32, 31, 39, 64, 3, 1), _both(({"64x64"}, {"128x32", "wgrad_128x64"})),
         [("last_m", "64x64", 43), ("whole", True), ("pix16", 11), ("odd",)]),
    Case("A train 128x32, last slab 43 rows", (3, 64, 31, 39, 32, 3, 1), _both(({"128x32"}, {"64x64", "wgrad_128x32"})),
         [("last_m", "128x32", 43), ("pix16", 11), ("odd",)]),
    Case("A train stride 2 to 127 x 159, parity backward", (4, 64, 254, 318, 128, 3, 2),
         {"f32": ({"64x128"}, {"parity", "64x64", "wgrad_128x64", "wgrad_group_sum"}),
          "bf16x3": ({"128x128_4x1"}, {"parity", "64x64", "wgrad_128x64", "wgrad_group_sum"})},
         [("last_m", "64x128", 4), ("last_m", "128x128_4x1", 4), ("pix16", 4), ("odd",)]),
    Case("B train split, Cout 132", (2, 256, 8, 10, 132, 3, 1),
         {"f32": ({"split_inkernel_stats"}, {"split_vec", "gathered", "wgrad_128x128"}),
          "bf16x3": ({"split_vec"}, {"split_vec", "gathered", "wgrad_128x128"})},
         [("valid_n", "split_inkernel_stats", 4), ("valid_n", "wgrad_128x128", 4), ("last_m", "split_inkernel_stats", 32)]),
    Case("C train 81 k-tiles over 8", (2, 144, 8, 10, 256, 3, 1),
         {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x64"})},
         [("splits", 8, True), ("last_m", "split_inkernel_stats", 32)]),
    Case("C train 81 k-tiles over 8, M 80", (1, 144, 8, 10, 256, 3, 1),
         {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x64"})},
         [("splits", 8, True), ("last_m", "split_inkernel_stats", 16)]),
    Case("C train 44 k-tiles over 5 with counters", (2, 704, 8, 10, 256, 1, 1),
         {"f32": ({"split_inkernel_stats"}, {"64x64", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"64x64", "wgrad_128x64"})},
         [("splits", 5, True), ("last_m", "split_inkernel_stats", 32)]),
    Case("C train M 189 over 8", (3, 256, 7, 9, 256, 3, 1),
         {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x128"}), "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x128"})},
         [("last_m", "split_inkernel_stats", 61), ("pix16", 13), ("odd",)]),
]
# the frlw_conv2d_fwd case of the same shape: in the integer mode the in-kernel and the two-launch reduction agree bit for bit
TWIN = {"C train 81 k-tiles over 8": "C 81 k-tiles over 8", "C train 81 k-tiles over 8, M 80": "C 81 k-tiles over 8, M 80",
        "C train 44 k-tiles over 5 with counters": "C 44 k-tiles, whole without counters", "C train M 189 over 8": "C M 189 over 8",
        "B train split, Cout 132": "B split, Cout 132"}

# ---- frlw_conv2d_dgrad with split-K scratch ------------------------------------------------------------------------------------------
DGRAD = [
    Case("C dgrad 144 k-tiles, Cin 144", (2, 144, 8, 10, 256, 3, 1), _both({"split_vec"}), [("dgrad_splits", 8, False), ("valid_n", "split_vec", 16)]),
    Case("C dgrad M 80", (1, 144, 8, 10, 256, 3, 1), _both({"split_vec"}), [("dgrad_splits", 8, False), ("last_m", "split_vec", 16)]),
    Case("C dgrad Cin 704", (2, 704, 8, 10, 256, 1, 1), _both({"64x64"}), [("last_m", "64x64", 32)]),
    Case("C dgrad M 189", (3, 256, 7, 9, 256, 3, 1), _both({"split_vec"}), [("last_m", "split_vec", 61), ("odd",)]),
    # E
    Case("E parity, 1 x 1 classes", (2, 16, 2, 2, 16, 3, 2), _both({"parity", "128x32"}), [("last_m", "128x32", 2), ("odd",)]),
    Case("E parity, ragged class tiles", (3, 32, 30, 38, 64, 3, 2), _both({"parity", "128x32"}), [("last_m", "128x32", 87), ("odd",)]),
    Case("E transposed gather 64x64, ragged", (2, 64, 31, 39, 64, 3, 2), _both({"64x64"}), [("last_m", "64x64", 50), ("odd",)]),
    Case("E stride 1, B 1", (1, 64, 9, 7, 64, 3, 1), _both({"64x64"}), [("last_m", "64x64", 63), ("odd",)]),
]

# ---- frlw_conv2d_wgrad: forms is the set, `part` the fraction of the scratch handed over -------------------------------------------
WCase = namedtuple("WCase", "name shape part forms claims")
WGRAD = [
    WCase("D M 63", (1, 16, 9, 7, 20, 3, 1), 1.0, {"wgrad_128x32"}, [("pix16", 15), ("last_r", "wgrad_128x32", 16), ("valid_n", "wgrad_128x32", 20), ("odd",)]),
    WCase("D 128x128, M 189 over 3 splits", (3, 256, 7, 9, 256, 3, 1), 1.0, {"wgrad_128x128"}, [("pix16", 13), ("wgrad_splits", 3), ("odd",)]),
    WCase("D six pixels per image", (8, 16, 2, 3, 32, 3, 1), 1.0, {"wgrad_128x32"}, [("short_image",), ("last_r", "wgrad_128x32", 16)]),
    WCase("D 1 x 1 maps, M 5", (5, 64, 1, 1, 64, 3, 1), 1.0, {"wgrad_128x64"}, [("short_image",), ("pix16", 5), ("odd",)]),
    WCase("D M 15", (1, 64, 3, 5, 64, 3, 1), 1.0, {"wgrad_128x64"}, [("short_image",), ("pix16", 15), ("odd",)]),
    WCase("D smallest Cin and Cout", (3, 4, 5, 3, 4, 1, 1), 1.0, {"wgrad_64x64"}, [("pix16", 13), ("last_r", "wgrad_64x64", 4), ("valid_n", "wgrad_64x64", 4), ("odd",)]),
    WCase("D stride 2, odd sizes", (2, 32, 15, 13, 64, 3, 2), 1.0, {"wgrad_128x64"}, [("last_r", "wgrad_128x64", 32)]),
    WCase("D group sums, M % 16 = 2", (2, 64, 63, 79, 64, 1, 1), 1.0, {"wgrad_64x64", "wgrad_group_sum"}, [("pix16", 2), ("wgrad_splits", 155), ("odd",)]),
    WCase("D a third of the scratch, M % 16 = 2", (2, 64, 63, 79, 64, 1, 1), 0.34, {"wgrad_64x64", "wgrad_scratch_limited"}, [("pix16", 2), ("odd",)]),
    WCase("B 128x128, Cout 132", (2, 256, 8, 10, 132, 3, 1), 1.0, {"wgrad_128x128"}, [("valid_n", "wgrad_128x128", 4), ("wgrad_splits", 2)]),
    # (not in the list the table was first drawn from: the wide tile's last row tile, 36 of 128 rows of R)
    WCase("D 128x128, R 2340", (2, 260, 5, 7, 256, 3, 1), 1.0, {"wgrad_128x128"}, [("last_r", "wgrad_128x128", 36), ("pix16", 6), ("odd",)]),
]

# ---- F: dx = data gradient + dx_add with rows wider than Cin, at a ragged tile -------------------------------------------------------
DX_ADD = Case("F dx_add, row pitch 80", (3, 64, 31, 39, 64, 3, 1),
              {"f32": ({"split_inkernel_stats"}, {"split_inkernel", "wgrad_128x64"}), "bf16x3": ({"split_vec"}, {"split_vec", "wgrad_128x64"})},
              [("last_m", "split_inkernel", 43), ("odd",)])
DX_ADD_PITCH, DX_ADD_OFFSET = 80, 8


def all_cases():
    return FWD + TRAIN + DGRAD + WGRAD + [DX_ADD]


def forms_of(case):
    """Every form a case names, whatever the precision and direction."""
    if isinstance(case, WCase):
        return set(case.forms)
    got = set()
    for v in case.forms.values():
        for s in (v if isinstance(v, tuple) else (v,)):
            got |= s
    return got
