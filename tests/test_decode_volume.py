# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_volume_tensors_device on the GPU: device-resident compressed volumes sampled at buffers of normalised
(u, v, w) triples with a level of detail per point into tensors.

Every case is bit for bit against the numpy model of the header's comment (tests/sample_volume_model.py) applied to what the
REFERENCE decoder writes for every whole level (the `ref` fixture, through the C ABI) -- never to anything the new call produced.
Every output buffer starts guard-filled and is compared whole; padded and tight pitches alternate, for the outputs, the triples
and the levels of detail (whose padding holds NaNs).  A chain is five levels of 20 x 14 x 9, 10 x 7 x 4, 5 x 3 x 2, 2 x 1 x 1 and
1 x 1 x 1 texels, every level a stream of its own with a constant-colour and a reserved-mode block where it has three blocks; the
footprints are 4x4, 6x6 and 8x5 over slices and 3x3x3, 4x4x3, 5x5x4 and 6x6x6: several blocks an axis with partial last blocks
on every axis, down to levels smaller than a block.  The grids are sample_volume_model.grid_inputs', whose reach
tests/test_decode_volume_cpu.py asserts on the model."""
import ctypes as C

import numpy as np
import pytest

import decode_cases as DC
import images
import sample_lod_model as L
import sample_model as S
import sample_volume_model as K
import tensor_model as M
from test_decode_regions import reference_decode
from test_decode_scaled import GUARD, SCALE, BIAS, dev, make_stream, type_of
from test_decode_sample import Source, contexts  # noqa: F401  (contexts: the fixture)
from test_decode_lod import grid_message, log_names

pytestmark = pytest.mark.gpu

FOOTPRINTS = {"x".join(str(v) for v in (f if f[2] > 1 else f[:2])): f for f in K.FOOTPRINTS_2D + K.FOOTPRINTS_3D}
FILTERS = (S.NEAREST, S.BILINEAR)
MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)


def make_volume_stream(product, A, block, dims, seed, special):
    """A W x H x D volume of noise on a gradient compressed at -fast: slice by slice for a 2D footprint (make_stream), as one
    image of 3D blocks otherwise; block 1 becomes a constant-colour block, block 2 a reserved mode."""
    w, h, d = dims
    if block[2] == 1:
        return make_stream(product, A, block[:2], w, h, depth=d, seed=seed, special=special)
    img = np.stack([np.roll(images.noisy(w, h, seed), 11 * z, axis=1) for z in range(d)])
    data = product.compress(img, block, A.PRE_FAST)
    b = data.reshape(-1, 16)
    assert b.shape[0] == int(np.prod([-(-n // s) for n, s in zip(dims, block)]))
    if special:
        b[1] = [0xFC, 0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x34, 0x12, 0xFF, 0xFF, 0x00, 0x80, 0xCD, 0xAB]
        b[2] = 0
    return data


def make_volume_chain(product, ref, A, block, dims, seed):
    """A Source per level of the sizes `dims` [(W, H, D)]."""
    chain = []
    for l, size in enumerate(dims):
        blocks = int(np.prod([-(-n // s) for n, s in zip(size, block)]))
        chain.append(Source(ref, A, block, size, make_volume_stream(product, A, block, size, seed + 7 * l, blocks >= 3)))
    return chain


@pytest.fixture(scope="module")
def chains(product, ref, A):
    """Per footprint: the chain of K.CHAIN."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_volume_chain(product, ref, A, FOOTPRINTS[name], K.CHAIN, 70 + len(made))
        return made[name]
    return get


@pytest.fixture(scope="module")
def pow2(product, ref, A):
    """Per footprint: levels of 16 x 8 x 8, 8 x 4 x 4 and 4 x 2 x 2 texels."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_volume_chain(product, ref, A, FOOTPRINTS[name], [(16, 8, 8), (8, 4, 4), (4, 2, 2)], 90 + len(made))
        return made[name]
    return get


class Out:
    """A guard-filled device buffer for one grid's tensor and device buffers of its triples and levels of detail, tight or with
    padded pitches."""

    def __init__(self, coords, lod, ttype, layout, channels, padded=False, coords_padded=False, lod_padded=False, front=64):
        import torch
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        oy, ox = coords.shape[:2]
        self.coords, self.lod, self.out, self.ttype, self.layout, self.channels, self.front, self.padded = coords, lod, (ox, oy), ttype, layout, channels, front, padded
        self.element = 4 if ttype == M.F32 else 2
        self.row = (ox if layout == M.PLANAR else ox * channels) + (3 if padded else 0)
        self.plane = self.row * oy + (5 if padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * channels if layout == M.PLANAR else self.row * oy
        self.buf = torch.full((front + elements * self.element + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + front
        # (the padding of a row of triples or of levels of detail holds NaNs: read into a point they would show)
        held = np.full((oy, 3 * ox + (5 if coords_padded else 0)), np.nan, dtype=np.float32)
        held[:, :3 * ox] = coords.reshape(oy, 3 * ox)
        self.cbuf = dev(held)
        self.crow = held.shape[1]
        self.coords_padded, self.lod_padded = coords_padded, lod_padded
        self.lbuf, self.lrow = None, 0
        if lod is not None:
            held = np.full((oy, ox + (5 if lod_padded else 0)), np.nan, dtype=np.float32)
            held[:, :ox] = lod
            self.lbuf = dev(held)
            self.lrow = held.shape[1]

    def grid(self, A, first_entry, level_count, bias, zero_pitches=False):
        pitches = (0, 0) if zero_pitches and not self.padded else (self.row, self.plane)
        crow = 0 if zero_pitches and not self.coords_padded else self.crow
        lrow = 0 if zero_pitches and not self.lod_padded else self.lrow
        return A.VolumeGrid(first_entry, level_count, self.out[0], self.out[1], self.cbuf.data_ptr(), crow, self.lbuf.data_ptr() if self.lbuf is not None else None, lrow,
                            bias, self.ptr, *pitches)

    def want(self, chain, sampler, bias, scale, fbias):
        want = np.full(self.buf.numel(), GUARD, dtype=np.uint8).view(M.BITS_DTYPE[self.ttype])
        s = K.sample(chain, sampler[0], sampler[1:4], sampler[4], self.coords, self.lod, bias)
        bits = M.convert(s[None], self.ttype, self.channels, scale, fbias)
        M.scatter(want, self.front // self.element, bits, self.layout, 0, self.row, self.row * self.out[1], self.plane)
        return want

    def got(self):
        return self.buf.cpu().numpy().view(M.BITS_DTYPE[self.ttype])

    def values(self):
        """The tight tensor's bits, [C, H, W] or [H, W, C], of an unpadded buffer."""
        assert not self.padded
        ox, oy = self.out
        n = ox * oy * self.channels
        flat = self.got()[self.front // self.element:self.front // self.element + n]
        return flat.reshape(self.channels, oy, ox) if self.layout == M.PLANAR else flat.reshape(oy, ox, self.channels)


def run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, cases, turn=0, what="", plain=False):
    """entries: ImageSetEntry per entry, texels: the reference's [D, H, W, 4] per entry; sampler: (filter, address_x, address_y,
    address_z, mip_filter); cases: [(first entry, levels, coords [H, W, 3], lod [H, W] or None, lod_bias)], all in one call.
    Returns the Outs (plain: none of them padded)."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    outs, grids = [], []
    for i, (first, count, coords, lod, bias) in enumerate(cases):
        o = Out(coords, lod, ttype, layout, channels, padded=not plain and (i + turn) % 2 == 1, coords_padded=(i + turn) % 4 >= 2, lod_padded=(i + turn) % 3 == 1)
        outs.append(o)
        grids.append(o.grid(A, first, count, bias, zero_pitches=(i + turn) % 3 == 0))
    err = product.sample_volume_tensors_device(ctx, entries, fmt, A.VolumeSampler(*sampler), grids)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    for o, (first, count, coords, lod, bias) in zip(outs, cases):
        chain = [texels[first + l] for l in range(count)]
        got, want = o.got(), o.want(chain, sampler, bias, scale32, bias32)
        if not np.array_equal(got, want):
            at = int(np.argwhere(got != want)[0][0])
            raise AssertionError("%s sampler %r grid %dx%d of entries %d..%d%s: first differing element at %d (row %d, plane %d): got 0x%x, want 0x%x; %d differ" %
                                 (what, sampler, o.out[0], o.out[1], first, first + count - 1, " padded" if o.padded else "", at - o.front // o.element, o.row, o.plane,
                                  got[at], want[at], int((got != want).sum())))
    return outs


def entries_of(chain, tname):
    return [s.entry(tname) for s in chain]


def texels_of(chain, profile, tname):
    return [s.texels(profile, tname) for s in chain]


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_generated_grids(product, A, contexts, chains, name):
    """The three grid shapes in one call under both filters and both mip filters, the address modes turning so that every axis has
    every mode; once more on level 0 alone (lod NULL), where a tile's pass lists more than a batch of blocks."""
    footprint = FOOTPRINTS[name]
    chain = chains(name)
    n = len(chain)
    ctx = contexts(footprint, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    assert [t.shape[:3][::-1] for t in texels] == K.CHAIN
    inputs = [K.grid_inputs(k, ox, oy, footprint) for k, (ox, oy) in enumerate(K.GRIDS)]
    seen = [set(), set(), set()]
    for filt in FILTERS:
        for mip in MIPS:
            turn = 2 * filt + mip
            address = (turn % 4, (3 * turn + 1) % 4, (turn + 2) % 4)
            for axis in range(3):
                seen[axis].add(address[axis])
            cases = [(0, n, coords, lod, 0.25 * k) for k, (coords, lod) in enumerate(inputs)]
            run_and_check(product, A, ctx, entries, texels, (filt,) + address + (mip,), (M.F16, M.PLANAR, 3), cases, turn=turn, what=name + " generated")
    assert all(s == {0, 1, 2, 3} for s in seen), seen
    cases = [(0, n, coords, None, 0.0) for coords, _ in inputs]
    run_and_check(product, A, ctx, entries, texels, (S.BILINEAR, S.REPEAT, S.MIRROR, S.REPEAT, L.MIP_NEAREST), (M.F32, M.INTERLEAVED, 4), cases, turn=1, what=name + " level 0")


@pytest.mark.parametrize("name", ["6x6", "4x4x3"])
def test_data_types_profiles_and_a_swizzle(product, ref, A, contexts, chains, name):
    """U8, F16 and F32 levels in one chain and one call; the four profiles (under HDR the reserved-mode block of an F16 level is
    NaN); the six tensor builds; then a BGRA and the Z swizzle on every level."""
    footprint = FOOTPRINTS[name]
    chain = chains(name)
    n = len(chain)
    names = [("u8", "f16", "f32")[l % 3] for l in range(n)]
    entries = [s.entry(t) for s, t in zip(chain, names)]
    formats = [(M.F32, M.PLANAR, 4), (M.F16, M.INTERLEAVED, 3), (M.BF16, M.PLANAR, 1), (M.F32, M.INTERLEAVED, 2), (M.F16, M.PLANAR, 4), (M.BF16, M.INTERLEAVED, 3)]
    for k, profile in enumerate((A.PRF_LDR, A.PRF_LDR_SRGB, A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)):
        ctx = contexts(footprint, profile)
        texels = [s.texels(profile, t) for s, t in zip(chain, names)]
        cases = [(0, n) + K.grid_inputs(20 + k, ox, oy, footprint) + (0.25 * i,) for i, (ox, oy) in enumerate(K.GRIDS[1:])]
        # (a chain of one level with a null lod: a volume without mips)
        cases.append((1, 1, K.grid_inputs(30 + k, 33, 3, footprint)[0], None, 0.0))
        sampler = (k % 2, (k + 1) % 4, (k + 2) % 4, k % 4, (k // 2) % 2)
        run_and_check(product, A, ctx, entries, texels, sampler, formats[k], cases, turn=k, what="types")
    ctx = contexts(footprint, A.PRF_LDR)
    for k, swz in enumerate(((A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A), (A.SWZ_R, A.SWZ_A, A.SWZ_Z, A.SWZ_1))):
        tname = ("u8", "f16")[k]
        entries = [A.compressed_entry(s.blocks, s.dims, type_of(A, tname), swz) for s in chain]
        texels = [reference_decode(ref, A, s.data, s.dims, footprint, A.PRF_LDR, {"u8": np.uint8, "f16": np.float16}[tname], swz) for s in chain]
        cases = [(0, n) + K.grid_inputs(40 + k, 19, 11, footprint) + (0.0,)]
        run_and_check(product, A, ctx, entries, texels, (S.BILINEAR, S.MIRROR, S.BORDER, S.CLAMP, L.MIP_LINEAR), formats[4 + k], cases, turn=k, what="swizzle")


def test_several_chains_in_one_call(product, A, contexts, chains, pow2):
    """Grids over two chains of different sizes and data types, and over parts of them, in one call."""
    a, b = chains("3x3x3"), pow2("3x3x3")
    ctx = contexts((3, 3, 3), A.PRF_LDR)
    entries = entries_of(a, "u8") + entries_of(b, "f16")
    texels = texels_of(a, A.PRF_LDR, "u8") + texels_of(b, A.PRF_LDR, "f16")
    na = len(a)
    cases = [(0, na) + K.grid_inputs(50, 33, 3, (3, 3, 3)) + (0.0,), (na, 3) + K.grid_inputs(51, 19, 11, (3, 3, 3), levels=3) + (0.5,),
             (1, 3) + K.grid_inputs(52, 70, 1, (3, 3, 3), levels=3) + (-0.25,), (na + 2, 1, K.grid_inputs(53, 19, 11, (3, 3, 3))[0], None, 0.0)]
    run_and_check(product, A, ctx, entries, texels, (S.BILINEAR, S.REPEAT, S.CLAMP, S.MIRROR, L.MIP_LINEAR), (M.F32, M.PLANAR, 4), cases, turn=2, what="several")


@pytest.mark.parametrize("block", [(6, 6), (3, 3, 3)], ids=DC.block_id)
def test_every_legal_encoding(product, ref, A, contexts, block):
    """The pool image of tests/decode_cases.py -- every block mode, partition count, plane count and endpoint format the footprint
    has -- as a volume (the 2D image stacked three slices deep), sampled at seeded points under both filters against the
    reference's decode: the list front end and the per-texel body decode every encoding the run decoder does, 3D blocks included."""
    stream = DC.streams(block)[-1]
    w, h, d = stream.dims
    block3 = tuple(block) + (1,) * (3 - len(block))
    stack = 3 if len(block) == 2 else 1
    data = np.tile(np.array(stream.data), stack)
    dims = (w, h, d * stack)
    rng = np.random.default_rng(17)
    coords = rng.uniform(0.0, 1.0, size=(97, 129, 3)).astype(np.float32)
    for profile, tname, out_type in (("PRF_LDR", "u8", np.uint8), ("PRF_HDR", "f16", np.float16)):
        one = DC.reference_decode(ref, A, stream, profile, out_type, "rgba", keep=False)
        want = np.concatenate([one] * stack)
        assert want.shape[:3] == dims[::-1]
        ctx = contexts(block3, getattr(A, profile))
        blocks = dev(data)                                       # (held here: the entry holds its address only)
        entry = A.compressed_entry(blocks, dims, type_of(A, tname))
        filt = S.BILINEAR if tname == "u8" else S.NEAREST
        run_and_check(product, A, ctx, [entry], [want], (filt, S.CLAMP, S.REPEAT, S.MIRROR, L.MIP_NEAREST), (M.F32, M.INTERLEAVED, 4), [(0, 1, coords, None, 0.0)],
                      what=stream.name + " " + profile)


def test_one_z_tap_gives_the_lod_call_bytes(product, A, contexts, chains, pow2):
    """On a context of a 2D footprint: under NEAREST any w inside slice kz, and under BILINEAR the slice centres of levels whose
    depths are powers of two (w D - 0.5 is an integer in every level the points use when the chain has one level), give the
    bytes astcenc_amd_sample_lod_tensors_device writes for z = kz."""
    import torch
    ctx = contexts((6, 6, 1), A.PRF_LDR)
    fmt_args = (M.F16, M.INTERLEAVED, 3)
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_INTERLEAVED, 3, SCALE, BIAS)
    rng = np.random.default_rng(8)
    uv = rng.uniform(-0.5, 1.5, size=(11, 19, 2)).astype(np.float32)
    lod = K.seeded_lods(rng, (11, 19), 3)

    def compare(entries, texels, first, count, filt, address, mip, w, kz, use_lod):
        coords = np.concatenate([uv, np.full(uv.shape[:2] + (1,), w, dtype=np.float32)], axis=-1)
        o = run_and_check(product, A, ctx, entries, texels, (filt,) + address + (mip,), fmt_args, [(first, count, coords, use_lod, 0.0)], what="one z tap", plain=True)[0]
        out = torch.full((11, 19, 3), 7.0, dtype=torch.float16, device="cuda")
        err = product.sample_lod_tensors_device(ctx, entries, fmt, (filt, address[0], address[1], mip), [(first, count, kz, dev(uv), dev(use_lod) if use_lod is not None else None, out)])
        assert err == A.SUCCESS, product.error_string(err)
        torch.cuda.synchronize()
        assert np.array_equal(o.values(), out.cpu().numpy().view(np.uint16)), (filt, mip, w, kz)

    # NEAREST over a chain whose levels all hold slice kz = 1: depths 8, 4, 2; w in [1/2, 1) is slice 1 of the coarsest only, so
    # the three levels go one by one, and two at once where the slices agree: w = 0.3 is slice 2 of 8 and 1 of 4
    chain = pow2("6x6")
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    for l, depth in enumerate((8, 4, 2)):
        for kz in (0, depth - 1):
            compare(entries, texels, l, 1, S.NEAREST, (S.REPEAT, S.BORDER, S.CLAMP), L.MIP_NEAREST, (kz + 0.3) / depth, kz, lod)
            compare(entries, texels, l, 1, S.BILINEAR, (S.MIRROR, S.CLAMP, S.BORDER), L.MIP_LINEAR, (kz + 0.5) / depth, kz, None)
    # the whole chain of 20 x 14 x 9 ...: w = 0 under CLAMP along z is slice 0 of every level under NEAREST, with every lambda
    chain = chains("6x6")
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    lod5 = K.seeded_lods(rng, (11, 19), 5)
    for mip in MIPS:
        compare(entries, texels, 0, 5, S.NEAREST, (S.REPEAT, S.MIRROR, S.CLAMP), mip, 0.0, 0, lod5)


@pytest.mark.parametrize("name", ["4x4", "3x3x3"])
def test_texel_centres_give_the_tensors_call_bytes(product, A, contexts, pow2, name):
    """Levels of 16 x 8 x 8, 8 x 4 x 4 and 4 x 2 x 2 texels: the texel centres of level l at lambda' = l give, under either filter
    and any address modes, the bytes astcenc_amd_decompress_tensors_device writes for the whole level -- F16 under the HDR
    profile, where the reserved-mode block is NaN and must stay in its own texels."""
    import torch
    footprint = FOOTPRINTS[name]
    chain = pow2(name)
    ctx = contexts(footprint, A.PRF_HDR)
    entries, texels = entries_of(chain, "f16"), texels_of(chain, A.PRF_HDR, "f16")
    assert np.isnan(texels[0].astype(np.float32)).any() and not np.isnan(texels[0].astype(np.float32)).all()
    fmt = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 4, SCALE, BIAS)
    for l, t in enumerate(texels):
        D, H, W = t.shape[:3]
        whole = torch.full((4, D, H, W), 7.0, dtype=torch.float32, device="cuda")
        err = product.decompress_tensors_device(ctx, entries, fmt, [(l, (0, 0, 0), (W, H, D), whole)])
        assert err == A.SUCCESS, product.error_string(err)
        torch.cuda.synchronize()
        whole = whole.cpu().numpy().view(np.uint32)
        centres = K.texel_centres(t)
        for filt in FILTERS:
            for mip in MIPS:
                sampler = (filt, (filt + mip) % 4, (l + 1) % 4, (2 * filt + mip + l) % 4, mip)
                o = run_and_check(product, A, ctx, entries, texels, sampler, (M.F32, M.PLANAR, 4), [(0, 3, centres, None, float(l))], what="centres", plain=True)[0]
                assert np.array_equal(o.values().reshape(4, D, H, W), whole), (l, filt, mip)


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, chains):
    """Every error the volume call adds to the lod call's, and those it shares, each with nothing written.  (Not among the cases:
    a `coords` on another device than entry 0's blocks -- on one GPU there is no such pointer to give.)"""
    import torch
    chain = chains("4x4x3")
    n = len(chain)
    ctx = contexts((4, 4, 3), A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((3, 40 * 40 * 4 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        c, lod = K.grid_inputs(1, 40, 40, (4, 4, 3))
        coords, lods = dev(c), dev(lod)
        cptr, lptr = coords.data_ptr(), lods.data_ptr()
        # first_entry, level_count, out_x, out_y, coords, coord_row_pitch, lod, lod_row_pitch, lod_bias, out, row_pitch, plane_pitch
        good = [A.VolumeGrid(0, n, 30, 20, cptr, 120, lptr, 40, 0.0, out[0].data_ptr(), 0, 0), A.VolumeGrid(1, 1, 40, 40, cptr, 0, lptr, 0, 0.5, out[1].data_ptr(), 0, 0),
                A.VolumeGrid(2, 3, 30, 40, cptr + 4, 117, None, 0, 1.0, out[2].data_ptr(), 0, 0)]
        entries = entries_of(chain, "u8")
        smp = A.VolumeSampler(A.SAMPLE_BILINEAR, 0, 1, 2, A.MIP_LINEAR)

        def call(fmt, grids, sampler=smp, entry_list=None, context=None):
            en = entry_list or entries
            arr = (A.ImageSetEntry * len(en))(*en)
            garr = (A.VolumeGrid * len(grids))(*grids)
            return product.lib.astcenc_amd_sample_volume_tensors_device(context or ctx, arr, len(en), C.byref(fmt) if fmt is not None else None,
                                                                        C.byref(sampler) if sampler is not None else None, garr, len(grids), None)

        def grid(index, **change):
            g = [A.VolumeGrid.from_buffer_copy(x) for x in good]
            for k, v in change.items():
                setattr(g[index], k, v)
            return g

        def entry(index, **change):
            en = [A.ImageSetEntry.from_buffer_copy(x) for x in entries]
            for k, v in change.items():
                setattr(en[index], k, v)
            return en

        fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
        cases = [
            # the volume call's own
            ("an unknown address_z", good, A.ERR_BAD_PARAM, "along z", dict(sampler=A.VolumeSampler(1, 0, 0, 4, 1))),
            ("a negative address_z", good, A.ERR_BAD_PARAM, "along z", dict(sampler=A.VolumeSampler(1, 0, 0, -1, 1))),
            ("coords not aligned to 4 bytes", grid(1, coords=cptr + 2), A.ERR_BAD_PARAM, grid_message(1, 3, "coords 0x... is not aligned to a float (4 bytes)"), {}),
            ("a coord_row_pitch below 3 out_x", grid(0, coord_row_pitch=89), A.ERR_BAD_PARAM, grid_message(0, 3, "coord_row_pitch 89: at least 90 floats"), {}),
            ("null coords", grid(2, coords=None), A.ERR_BAD_CONTEXT, grid_message(2, 3, "coords is null"), {}),
            ("a level deeper than 65536", good, A.ERR_BAD_PARAM, "grid 0 of 3", dict(entry_list=entry(1, dim_x=4, dim_y=4, dim_z=65537, blocks_len=21846 * 16))),
            ("a level wider than 65536", good, A.ERR_BAD_PARAM, "grid 0 of 3", dict(entry_list=entry(1, dim_x=65537, dim_y=4, dim_z=3, blocks_len=16385 * 16))),
            # (65536 x 65536 x 3 at 4x4x3 is 2^28 blocks: counted with dim_z it would be refused, counted in layers it is a level
            #  like any other -- the call gets as far as the device check of its 16-byte stream; 65536^2 x 48 is 2^32 blocks)
            ("an entry of 2^32 blocks", good, A.ERR_BAD_PARAM, "entry 1 of %d" % n, dict(entry_list=entry(1, dim_x=65536, dim_y=65536, dim_z=48, blocks_len=(1 << 32) * 16))),
            # shared with the lod call
            ("a null sampler", good, A.ERR_BAD_PARAM, "sampler", dict(sampler=None)),
            ("an unknown mip filter", good, A.ERR_BAD_PARAM, "mip_filter", dict(sampler=A.VolumeSampler(1, 0, 0, 0, 2))),
            ("an unknown filter", good, A.ERR_BAD_PARAM, "filter", dict(sampler=A.VolumeSampler(2, 0, 0, 0, 0))),
            ("an unknown address_y", good, A.ERR_BAD_PARAM, "address modes", dict(sampler=A.VolumeSampler(1, 0, 4, 0, 0))),
            ("no levels", grid(1, level_count=0), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("too many levels", grid(1, level_count=33), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("levels beyond the entries", grid(2, first_entry=n - 1), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("an infinite lod_bias", grid(2, lod_bias=float("inf")), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("a lod not aligned to 4 bytes", grid(1, lod=lptr + 2), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("a lod_row_pitch below out_x", grid(0, lod_row_pitch=29), A.ERR_BAD_PARAM, "grid 0 of 3", {}),
            ("a zero out_x", grid(1, out_x=0), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("an out_y above 65535", grid(1, out_y=65536), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("a row pitch below the output's", grid(2, row_pitch=29), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("a null out", grid(2, out=None), A.ERR_BAD_CONTEXT, "grid 2 of 3", {}),
            ("a stream shorter than the level", good, A.ERR_OUT_OF_MEM, "entry 0 of %d" % n, dict(entry_list=entry(0, blocks_len=16))),
        ]
        for what, grids, code, named, kw in cases:
            del logged[:]
            assert call(fmt, grids, **kw) == code, (what, logged)
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(log_names(named, m) for m in logged), (what, logged)
        assert call(None, good) == A.ERR_BAD_PARAM
        # coordinates and levels of detail are data: none of them is an error -- and the good call is good (a null lod, triples
        # that start on an odd float and an odd pitch included)
        assert call(fmt, good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:, :64] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
    # the three predecessors still refuse a context of a 3D footprint
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    o = torch.full((3, 4, 4), 7.0, dtype=torch.float16, device="cuda")
    uv = dev(np.zeros((4, 4, 2), dtype=np.float32))
    assert product.sample_lod_tensors_device(ctx, entries, fmt, (1, 0, 0, 1), [(0, 1, 0, uv, None, o)]) == A.ERR_BAD_PARAM
    assert product.sample_tensors_device(ctx, entries, fmt, (1, 0, 0), [(0, 0, uv, o)]) == A.ERR_BAD_PARAM
