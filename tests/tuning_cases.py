# SPDX-License-Identifier: Apache-2.0
"""Shared by tests/test_tuning_fields_cpu.py and tests/test_tuning_fields.py: the hand-set fields of astcenc_config -- the 16
tune_* fields, the four channel weights and rgbm_m_scale -- that a caller may edit between astcenc_config_init and
astcenc_context_alloc, each at the ends of its valid range, at one interior value, outside the range where validate_config
(csrc/astcenc_entry.cpp) clamps, and, for the float fields, at NaN and +inf.

Not a conftest and not a test module: a plain module, imported by name.  Nothing here is random at run time.

A case is (field, value, kind, base, image):
  base   a key of BASES: (profile, block, quality, flags); the base tweak of a case is base_tweak(field) -- the fields that
         act only inside the two- to four-partition search get tune_partition_count_limit = 4, so that the search runs
  image  a key of IMAGES: a generator of a 36-block image for the base's footprint
  kind   "lo" / "hi": the ends of the valid range; "mid": an interior value (no preset's, where the range allows that);
         "below" / "above": outside the range, the reference clamps it to the "lo" / "hi" value;
         "nan": validate_config's `a > b ? a : b` turns it into the lower clamp where there is one;
         "side": tune_search_mode0_enable, which has no range but a threshold: a value on the other side of 0.85 than the
                 base context's must bite, one on the same side must change nothing;
         "inert": a field the context does not read (tune_db_limit in an HDR profile, where context_alloc sets it to 0;
                  tune_search_mode0_enable and tune_block_mode_limit on a 3D footprint): the reference's bytes must NOT change.

IMAGE_OF names, per (field, base), the image on which the reference's bytes show that the field bites; bites.txt
(profiles/tuning_fields, written by `python tests/tuning_cases.py`) records the count of differing blocks of every case.
NOT_SHOWN lists the (field, direction) pairs that no case makes bite, QUIET the single cases that do not although their
field does on another footprint or value.

Where to add a case: a new field or value goes into VALUES; run `python tests/tuning_cases.py probe`, which prints the
IMAGE_OF entries and the QUIET candidates for the table as it stands, then `python tests/tuning_cases.py` for bites.txt."""
import collections
import itertools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":      # (as a test module's import the paths are conftest.py's)
    sys.path[:0] = [os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle")]

import astcenc_amd as A  # noqa: E402
import encoding_cases as E  # noqa: E402
import images  # noqa: E402

BITES = os.path.join(ROOT, "profiles", "tuning_fields", "bites.txt")
NAN, INF = float("nan"), float("inf")
K = "astc_compress_blocks_"

BASES = collections.OrderedDict([
    ("ldr6x6", (A.PRF_LDR, (6, 6), A.PRE_MEDIUM, 0)),                   # 36 texels
    ("ldr10x8", (A.PRF_LDR, (10, 8), A.PRE_MEDIUM, 0)),                 # 80 texels: a 64-lane trip and a 16-lane tail
    ("ldr5x5x5", (A.PRF_LDR, (5, 5, 5), A.PRE_MEDIUM, 0)),              # 125 texels, odd
    ("hdr6x6", (A.PRF_HDR, (6, 6), A.PRE_MEDIUM, 0)),
    ("rgbm6x6", (A.PRF_LDR, (6, 6), A.PRE_MEDIUM, A.FLG_MAP_RGBM)),
    ("ldr8x8t", (A.PRF_LDR, (8, 8), A.PRE_THOROUGH, 0)),                # (the second fixed-context build: test_tuning_fields.py)
])

INT_FIELDS = ["tune_partition_count_limit", "tune_2partition_index_limit", "tune_3partition_index_limit", "tune_4partition_index_limit",
              "tune_block_mode_limit", "tune_refinement_limit", "tune_candidate_limit", "tune_2partitioning_candidate_limit",
              "tune_3partitioning_candidate_limit", "tune_4partitioning_candidate_limit"]
FLOAT_FIELDS = ["tune_db_limit", "tune_mse_overshoot", "tune_2partition_early_out_limit_factor", "tune_3partition_early_out_limit_factor",
                "tune_2plane_early_out_limit_correlation", "tune_search_mode0_enable"]
WEIGHT_FIELDS = ["cw_r_weight", "cw_g_weight", "cw_b_weight", "cw_a_weight"]
FIELDS = INT_FIELDS + FLOAT_FIELDS + WEIGHT_FIELDS + ["rgbm_m_scale"]
# fields read only by the search over two to four partitions: their base contexts try four partitions
PARTITION_FIELDS = [f for f in FIELDS if "partition_index" in f or "partitioning" in f or "partition_early" in f]

# field -> [(value, kind)]; the first "lo" / "hi" value is the clamp edge of the "below" / "above" values
_index = [(1, "lo"), (1024, "hi"), (7, "mid"), (0, "below"), (5000, "above")]
_cands = [(1, "lo"), (8, "hi"), (7, "mid"), (0, "below"), (13, "above")]
_factor = [(0.0, "lo"), (INF, "hi"), (0.5, "mid"), (-1.0, "below"), (NAN, "nan")]
# A channel weight below a thousandth of the largest is raised to that: with the other three at 1 (2 * rgbm_m_scale for
# alpha under MAP_RGBM is not among the bases of these fields) the lower edge is float32(1) / float32(1000).
_WEIGHT_EDGE = float(np.float32(1.0) / np.float32(1000.0))
_weight = [(_WEIGHT_EDGE, "lo"), (1e30, "hi"), (0.37, "mid"), (0.0, "below"), (-1.0, "below")]
VALUES = collections.OrderedDict([
    ("tune_partition_count_limit", [(1, "lo"), (4, "hi"), (2, "mid"), (0, "below"), (9, "above")]),     # (2 and 3 are both presets')
    ("tune_2partition_index_limit", _index),
    ("tune_3partition_index_limit", _index),
    ("tune_4partition_index_limit", _index),
    ("tune_block_mode_limit", [(1, "lo"), (100, "hi"), (50, "mid"), (0, "below"), (250, "above")]),
    ("tune_refinement_limit", [(1, "lo"), (5, "mid"), (9, "mid"), (20, "mid"), (0, "below")]),          # (no upper clamp)
    ("tune_candidate_limit", [(1, "lo"), (8, "hi"), (5, "mid"), (0, "below"), (13, "above")]),
    ("tune_2partitioning_candidate_limit", _cands),
    ("tune_3partitioning_candidate_limit", _cands),
    ("tune_4partitioning_candidate_limit", _cands),
    ("tune_db_limit", [(0.0, "lo"), (INF, "hi"), (30.0, "mid"), (-1.0, "below"), (NAN, "nan")]),
    ("tune_mse_overshoot", [(1.0, "lo"), (INF, "hi"), (2.0, "mid"), (0.5, "below"), (NAN, "nan")]),
    ("tune_2partition_early_out_limit_factor", _factor),
    ("tune_3partition_early_out_limit_factor", _factor),
    ("tune_2plane_early_out_limit_correlation", _factor),
    # no clamp; the search reads it as `>= 0.85` (csrc/wave_block.h): both sides of the threshold (the presets hold 0 or 1, so
    # one of the two is the base's side and must change nothing) and the two non-finite values
    ("tune_search_mode0_enable", [(0.84, "side"), (0.86, "side"), (NAN, "nan"), (INF, "side")]),
    ("cw_r_weight", _weight), ("cw_g_weight", _weight), ("cw_b_weight", _weight), ("cw_a_weight", _weight),
    ("rgbm_m_scale", [(1.0, "lo"), (20.0, "hi"), (3.0, "mid"), (0.0, "below")]),
])
assert list(VALUES) == FIELDS


def base_tweak(field):
    return {"tune_partition_count_limit": 4} if field in PARTITION_FIELDS else {}


def bases_of(field):
    """The base contexts of a field's single-field cases."""
    if field == "rgbm_m_scale":
        return ["rgbm6x6"]
    return ["ldr6x6", "ldr10x8", "ldr5x5x5", "hdr6x6"]


def inert(field, base):
    """Fields the base's context does not read: context_alloc sets tune_db_limit to 0 in an HDR profile; the search looks at
    tune_search_mode0_enable for 2D footprints only; a 3D footprint keeps every block mode (no percentile table)."""
    return (field, base) in (("tune_db_limit", "hdr6x6"), ("tune_search_mode0_enable", "ldr5x5x5"), ("tune_block_mode_limit", "ldr5x5x5"))


# ---- images: 36 blocks each ----------------------------------------------------------------------------------------------

def _crop(img, block):
    """The first 6 x 6 blocks of a 2D image, the first 4 x 3 x 3 of a volume."""
    if len(block) > 2:
        return np.ascontiguousarray(img[:3 * block[2], :3 * block[1], :4 * block[0]])
    return np.ascontiguousarray(img[:6 * block[1], :6 * block[0]])


def _noisy(block, seed=5):
    if len(block) > 2:
        return np.stack([images.noisy(4 * block[0], 3 * block[1], seed + z) for z in range(3 * block[2])])
    return images.noisy(6 * block[0], 6 * block[1], seed)


def _hdr_noisy(block):
    return A.synthetic_hdr_image(6 * block[0], 6 * block[1], 3)


def _low_m(block):
    from test_gpu_parity import low_m_image
    return low_m_image(np.random.default_rng(17), (6 * block[0], 6 * block[1]))


IMAGES = collections.OrderedDict([
    ("patches2", lambda b: _crop(E.patches(b, 2, 31), b)),
    ("patches3", lambda b: _crop(E.patches(b, 3, 32), b)),
    ("patches4", lambda b: _crop(E.patches(b, 4, 33), b)),
    ("mixed4", lambda b: _crop(E.mixed_patches(b, 4, 90), b)),
    ("noisy", _noisy),
    ("two_colour", lambda b: _crop(E.two_colour(b, 48), b)),
    ("lone_a", lambda b: _crop(E.lone_channel(b, 3, 44), b)),
    ("hdr_patches2", lambda b: _crop(E.hdr_patches(b, 2, 51), b)),
    ("hdr_patches3", lambda b: _crop(E.hdr_patches(b, 3, 52), b)),
    ("hdr_patches4", lambda b: _crop(E.hdr_patches(b, 4, 53), b)),
    ("hdr_mixed4", lambda b: _crop(E.mixed_patches(b, 4, 94, hdr=True), b)),
    ("hdr_noisy", _hdr_noisy),
    ("hdr_lone_a", lambda b: _crop(E.lone_channel(b, 3, 61, hdr=True), b)),
    ("low_m", _low_m),
    ("pastel", lambda b: _crop(E.pastel(b, 84), b)),
    ("l_noise", lambda b: _crop(E.noise(b, 40, "l"), b)),
    ("rgb_noise", lambda b: _crop(E.noise(b, 38, "rgb"), b)),
    ("hdr_mixed3", lambda b: _crop(E.mixed_patches(b, 3, 93, hdr=True), b)),
    ("hdr_rgb_ramps", lambda b: _crop(E.ramps(b, 92, "rgb", hdr=True), b)),
    ("hdr_gray_ramps", lambda b: _crop(E.ramps(b, 91, "l", hdr=True), b)),
])
LDR_IMAGES = ["patches4", "patches3", "patches2", "mixed4", "noisy", "two_colour", "lone_a", "pastel", "l_noise", "rgb_noise"]
HDR_IMAGES = ["hdr_patches4", "hdr_patches3", "hdr_patches2", "hdr_mixed4", "hdr_noisy", "hdr_lone_a", "hdr_mixed3", "hdr_rgb_ramps", "hdr_gray_ramps"]

_IMAGE_CACHE = {}


def image(name, block):
    key = (name, tuple(block))
    if key not in _IMAGE_CACHE:
        img = np.ascontiguousarray(IMAGES[name](tuple(block)))
        bz = block[2] if len(block) > 2 else 1
        blocks = -(-img.shape[-2] // block[0]) * -(-img.shape[-3] // block[1]) * (-(-img.shape[0] // bz) if img.ndim == 4 else 1)
        assert blocks == 36, (key, blocks)
        img.setflags(write=False)
        _IMAGE_CACHE[key] = img
    return _IMAGE_CACHE[key]


def candidate_images(base):
    """The images tried for a base context (python tests/tuning_cases.py probe)."""
    if base == "rgbm6x6":
        return ["low_m", "noisy", "patches3"]
    return HDR_IMAGES if base == "hdr6x6" else LDR_IMAGES


# (field, base[, value]) -> the image on which the field's values bite in the reference (chosen by `python tests/tuning_cases.py
# probe`: the first candidate image on which most of the field's in-range values change at least one block, and for a value
# that changes none there, the first image on which it does); "*" is the default per base
IMAGE_OF = {
    "*": {"ldr6x6": "patches4", "ldr10x8": "patches4", "ldr5x5x5": "patches4", "hdr6x6": "hdr_patches4", "rgbm6x6": "low_m", "ldr8x8t": "patches4"},
    ("tune_3partition_index_limit", "hdr6x6"): "hdr_patches3",
    ("tune_4partition_index_limit", "ldr6x6"): "rgb_noise",
    ("tune_4partition_index_limit", "ldr10x8"): "l_noise",
    ("tune_4partition_index_limit", "ldr5x5x5"): "l_noise",
    ("tune_4partition_index_limit", "hdr6x6"): "hdr_mixed3",
    ("tune_refinement_limit", "ldr6x6"): "patches2",
    ("tune_refinement_limit", "ldr5x5x5"): "patches3",
    ("tune_refinement_limit", "hdr6x6"): "hdr_patches2",
    ("tune_candidate_limit", "hdr6x6"): "hdr_patches3",
    ("tune_2partitioning_candidate_limit", "ldr6x6"): "l_noise",
    ("tune_3partitioning_candidate_limit", "ldr6x6"): "mixed4",
    ("tune_3partitioning_candidate_limit", "ldr10x8"): "mixed4",
    ("tune_3partitioning_candidate_limit", "ldr5x5x5"): "mixed4",
    ("tune_3partitioning_candidate_limit", "hdr6x6"): "hdr_mixed4",
    ("tune_db_limit", "ldr6x6"): "pastel",
    ("tune_db_limit", "ldr10x8"): "noisy",
    ("tune_db_limit", "ldr5x5x5"): "noisy",
    ("tune_mse_overshoot", "ldr6x6"): "pastel",
    ("tune_mse_overshoot", "ldr10x8"): "pastel",
    ("tune_mse_overshoot", "ldr5x5x5"): "noisy",
    ("tune_mse_overshoot", "ldr5x5x5", INF): "pastel",
    ("tune_2partition_early_out_limit_factor", "ldr6x6"): "l_noise",
    ("tune_2partition_early_out_limit_factor", "ldr10x8"): "patches3",
    ("tune_2partition_early_out_limit_factor", "ldr5x5x5"): "patches3",
    ("tune_2partition_early_out_limit_factor", "hdr6x6"): "hdr_mixed3",
    ("tune_2plane_early_out_limit_correlation", "ldr6x6"): "lone_a",
    ("tune_2plane_early_out_limit_correlation", "ldr10x8"): "lone_a",
    ("tune_2plane_early_out_limit_correlation", "ldr5x5x5"): "lone_a",
    ("tune_2plane_early_out_limit_correlation", "hdr6x6"): "hdr_rgb_ramps",
    ("tune_search_mode0_enable", "ldr6x6"): "lone_a",
    ("tune_search_mode0_enable", "ldr10x8"): "lone_a",
    ("tune_search_mode0_enable", "hdr6x6"): "hdr_gray_ramps",
    ("cw_a_weight", "ldr6x6"): "patches3",
    ("cw_a_weight", "ldr10x8"): "patches3",
    ("cw_a_weight", "ldr5x5x5"): "patches3",
}

# (field, direction) -> what was tried.  direction: "down" / "up", the value against the base context's.  No case of the
# table makes these change a byte of the reference's output; tests/test_tuning_fields_cpu.py fails when one does.
_TRIED = "candidate_images() of every base of the field (6x6, 10x8, 5x5x5 LDR and 6x6 HDR, 36 blocks each, -medium)"
NOT_SHOWN = {
    ("tune_4partitioning_candidate_limit", "down"): _TRIED,
    ("tune_4partitioning_candidate_limit", "up"): _TRIED,
    ("rgbm_m_scale", "down"): "1 and 3 against the flag's 5 with FLG_MAP_RGBM at 6x6 -medium on low_m, noisy, patches3",
    ("rgbm_m_scale", "up"): "20 against the flag's 5 with FLG_MAP_RGBM at 6x6 -medium on low_m, noisy, patches3",
}
# In-range cases that change no block of the reference's output on any candidate image of their base, although their
# (field, direction) does on another base or value: they run for parity only.  tests/test_tuning_fields_cpu.py fails when one
# of them bites (python tests/tuning_cases.py probe lists them).
QUIET = {
    "tune_4partition_index_limit=7-hdr6x6-hdr_mixed3",
    "tune_mse_overshoot=1-hdr6x6-hdr_patches4",
    "tune_mse_overshoot=inf-hdr6x6-hdr_patches4",
    "tune_mse_overshoot=2-hdr6x6-hdr_patches4",
    "tune_2plane_early_out_limit_correlation=inf-ldr5x5x5-lone_a",
}
MAX_NOT_SHOWN = 6
MAY_BE_SILENT = ("tune_4partitioning_candidate_limit", "rgbm_m_scale")       # every other field bites in at least one direction


Case = collections.namedtuple("Case", "field value kind base image")


def case_id(c):
    return "%s=%s-%s-%s" % (c.field, ("%g" % c.value) if isinstance(c.value, float) else c.value, c.base, c.image)


def context_of(c):
    """(profile, block, quality, flags, tweak dict) of a case or combination."""
    profile, block, quality, flags = BASES[c.base]
    tweak = dict(base_tweak(c.field))
    tweak[c.field] = c.value
    return profile, block, quality, flags, tweak


def base_context_of(c):
    profile, block, quality, flags = BASES[c.base]
    return profile, block, quality, flags, dict(base_tweak(c.field))


def image_of(field, base, value=None):
    return IMAGE_OF.get((field, base, value), IMAGE_OF.get((field, base), IMAGE_OF["*"][base]))


def cases(bases=None):
    out = []
    for field in FIELDS:
        for base in (bases_of(field) if bases is None else bases):
            for value, kind in VALUES[field]:
                # (a value outside the range runs on the image of the edge it is clamped to)
                edge = [v for v, k in VALUES[field] if k == {"below": "lo", "above": "hi"}.get(kind)]
                out.append(Case(field, value, "inert" if inert(field, base) else kind, base, image_of(field, base, edge[0] if edge else value)))
    return out


def cases_of(field):
    return [c for c in cases() if c.field == field]


def clamp_edge(c):
    """The in-range case an out-of-range case must equal in the reference."""
    want = "lo" if c.kind == "below" else "hi"
    edge = [v for v, k in VALUES[c.field] if k == want][0]
    return c._replace(value=edge, kind=want)


def direction(value, base_value):
    """"down" / "up" of a value against the base context's; None where it is the same (or NaN)."""
    if isinstance(value, float) and math.isnan(value):
        return None
    return "down" if value < base_value else ("up" if value > base_value else None)


def config_value(lib, c, field=None):
    """The field's value in the base context's config (read from `lib`'s astcenc_config_init)."""
    profile, block, quality, flags = BASES[c.base]
    err, cfg = lib.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, quality, flags)
    assert err == 0
    for f, v in base_tweak(c.field).items():
        setattr(cfg, f, v)
    return getattr(cfg, field or c.field)


# ---- combinations: what the LDS layout is sized from, at its corners -------------------------------------------------------
# The smallest and the largest texel count of every generic class: ldr64 takes up to 64 texels (4x4, 8x8; 10x5 with its 50
# texels is one of its footprints too, not the smallest of `ldr`, which is 10x8), ldr the rest up to 12x12.
COMBO_FOOTPRINTS = [(A.PRF_LDR, (4, 4), "ldr64"), (A.PRF_LDR, (8, 8), "ldr64"), (A.PRF_LDR, (10, 5), "ldr64"), (A.PRF_LDR, (10, 8), "ldr"),
                    (A.PRF_LDR, (12, 12), "ldr"), (A.PRF_LDR, (6, 6, 6), "3d"), (A.PRF_HDR, (6, 6), "hdr64"), (A.PRF_HDR, (12, 12), "hdr")]
COMBO_PRESETS = [A.PRE_FASTEST, A.PRE_THOROUGH]
COMBO_CORNERS = list(itertools.product((1, 8), (1, 4), (1, 1024), (1, 100)))     # candidates, partitions, index limit, mode limit

Combo = collections.namedtuple("Combo", "profile block quality flags tweak image build_class")


def corner_tweak(candidates, partitions, index_limit, modes):
    return {"tune_candidate_limit": candidates, "tune_partition_count_limit": partitions, "tune_2partition_index_limit": index_limit,
            "tune_3partition_index_limit": index_limit, "tune_4partition_index_limit": index_limit, "tune_block_mode_limit": modes}


def combos():
    out = []
    for profile, block, cls in COMBO_FOOTPRINTS:
        for quality in COMBO_PRESETS:
            for corner in COMBO_CORNERS:
                out.append(Combo(profile, block, quality, 0, corner_tweak(*corner), "hdr_patches4" if profile == A.PRF_HDR else "patches4", cls))
    return out


def combo_id(c):
    t = c.tweak
    return "%s%s-q%g-c%d-p%d-i%d-m%d" % ("hdr" if c.profile == A.PRF_HDR else "ldr", "x".join(map(str, c.block)), c.quality,
                                          t["tune_candidate_limit"], t["tune_partition_count_limit"], t["tune_2partition_index_limit"],
                                          t["tune_block_mode_limit"])


def generic_kernel(profile, block):
    """The generic build of a context no fixed-context build accepts (csrc/backend_hip.hip, kernel_variants): by profile and by
    texel count -- a volume runs the build of its texel count."""
    hdr = profile in (A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)
    texels = block[0] * block[1] * (block[2] if len(block) > 2 else 1)
    return K + ("hdr" if hdr else "ldr") + ("64" if texels <= 64 else "")


FIXED_KERNELS = {"ldr6x6": K + "ldr_6x6m", "ldr8x8t": K + "ldr_8x8t", "hdr6x6": K + "hdr_6x6m"}


def expected_kernel(c):
    """The build a case's context runs with run-time builds off: the generic one of its class -- unless the case changes no
    record of a context that has a fixed-context build (a field the context does not read, no base tweak)."""
    if c.kind == "inert" and c.base in FIXED_KERNELS and not base_tweak(c.field):
        return FIXED_KERNELS[c.base]
    return generic_kernel(BASES[c.base][0], BASES[c.base][1])


def build_class(profile, block, quality, tweak):
    """encoding_cases.build_class for a context with hand-set fields: a fixed-context build serves its context only with every
    record as the preset left it."""
    cls = E.build_class(profile, block, quality)
    if tweak and cls in ("ldr_6x6m", "ldr_8x8t", "hdr_6x6m"):
        return ("hdr" if cls.startswith("hdr") else "ldr") + "64"
    return cls


# ---- running ------------------------------------------------------------------------------------------------------------------

def apply(tweak):
    def edit(cfg):
        for f, v in tweak.items():
            assert hasattr(cfg, f), f
            setattr(cfg, f, v)
    return edit if tweak else None


def compress(lib, ctx, img, **kw):
    profile, block, quality, flags, tweak = ctx
    return lib.compress(img, block, quality, profile=profile, flags=flags, tweak=apply(tweak), **kw).reshape(-1, 16)


def differing(a, b):
    return int((a.reshape(-1, 16) != b.reshape(-1, 16)).any(axis=1).sum())


class Outputs:
    """One library's bytes per (context, image), compressed once per session and never changed."""

    def __init__(self, lib):
        self.ref, self.bytes = lib, {}

    def want(self, ctx, image_name):
        profile, block, quality, flags, tweak = ctx
        key = (profile, tuple(block), quality, flags, tuple(sorted((f, repr(v)) for f, v in tweak.items())), image_name)
        if key not in self.bytes:
            out = compress(self.ref, ctx, image(image_name, block))
            out.setflags(write=False)
            self.bytes[key] = out
        return self.bytes[key]

    def bite(self, c):
        """Blocks of the case's image that the case's value changes against the base context's bytes."""
        return differing(self.want(context_of(c), c.image), self.want(base_context_of(c), c.image))


def _main(argv):
    import oracle_libs as O
    ref = Outputs(A.Library(O.LIB_REF_NONE))
    if argv[1:] == ["probe"]:
        # per (field, base): the image on which most in-range values bite; per value that does not bite there, the first that does
        image_of, quiet = [], []
        for field in FIELDS:
            for base in bases_of(field):
                if inert(field, base):
                    continue
                values = [(v, k) for v, k in VALUES[field] if k not in ("below", "above")]
                rows = [(name, [ref.bite(Case(field, v, k, base, name)) for v, k in values]) for name in candidate_images(base)]
                best = max(rows, key=lambda r: sum(1 for n in r[1] if n))
                if best[0] != IMAGE_OF["*"][base]:
                    image_of.append("    (%r, %r): %r," % (field, base, best[0]))
                for i, (v, k) in enumerate(values):
                    if best[1][i] or (isinstance(v, float) and math.isnan(v)):
                        continue
                    other = [name for name, counts in rows if counts[i]]
                    if other:
                        image_of.append("    (%r, %r, %r): %r," % (field, base, v, other[0]))
                    else:
                        quiet.append("    %r," % case_id(Case(field, v, k, base, best[0])))
                print("%-44s %-9s %s" % (field, base, "  ".join("%s:%s" % r for r in rows)), flush=True)
        print("IMAGE_OF\n" + "\n".join(image_of) + "\nQUIET\n" + "\n".join(quiet))
        return
    lines = ["# blocks (of 36) of the case's image that the reference encodes differently from the base context's bytes; for a",
             "# value outside the valid range: from the bytes at the clamp edge.  Written by `python tests/tuning_cases.py`.",
             "# %-58s %-6s %s" % ("case", "kind", "blocks")]
    for c in cases():
        n = differing(ref.want(context_of(c), c.image), ref.want(context_of(clamp_edge(c)), c.image)) if c.kind in ("below", "above") else ref.bite(c)
        lines.append("%-60s %-6s %d" % (case_id(c), c.kind, n))
    os.makedirs(os.path.dirname(BITES), exist_ok=True)
    with open(BITES, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote %s: %d cases" % (os.path.relpath(BITES, ROOT), len(lines) - 3))


if __name__ == "__main__":
    _main(sys.argv)
