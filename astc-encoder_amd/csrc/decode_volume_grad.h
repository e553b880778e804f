// SPDX-License-Identifier: Apache-2.0
// The gradients of the volume sampler (astcenc_amd_sample_volume_grad_device): for every point of a grid and an upstream
// gradient of the forward call's output, d loss / d (u, v, w) and d loss / d lambda -- the vector-Jacobian product of
// astcenc_amd_sample_volume_tensors_device with respect to its coordinates and levels of detail; the texels are compressed and
// fixed (include/astcenc_amd.h has the definition, tests/sample_volume_grad_model.py spells it out in numpy).
//
// What decode_lod_grad.h is to decode_lod.h, this header is to decode_volume.h: a work item is a tile of 64 points of one grid,
// the lane is the point, and the level walk is written out again with the gradient's levels -- the forward call's and, where
// grad_lod is wanted and lambda' is not clamped under MIP_LINEAR, level l0 + 1 even when its weight is zero.  A level pass is
// decode_volume.h's pipeline (its eight-slot sample_batches, untouched) with a tap former that keeps all eight taps under BILINEAR:
// the difference along an axis needs both indices of that axis even where the forward tap 1 has weight zero.  After the batches
// the lane forms the forward sample (sample_point_sums(VolumePoint): the taps of weight zero are not in it), the difference
// sums along x, y and z one channel at a time and, with the upstream gradient, the four binary64 values it keeps of the level:
// Dx, Dy, Dz and S.  After the last pass the lane blends (two products and a sum, one rounding) and stores the triple with
// three 4-byte stores and the level-of-detail gradient with one.
//
// Included by kernel_decode_volume_grad.hip and tests/harness/decode_volume_grad_check.cpp only.
//
// Layout: decode_lod.h's with DecodeVolumeGradRecord in the place of DecodeLodRecord: ImageSetTable (count = grids, total =
// tiles), first[count], padding, DecodeVolumeGradRecord[count], then the DecodeLodLevel records of grid 0's levels, of grid 1's ...
#pragma once
#include "decode_volume.h"
#include "decode_lod_grad.h"

namespace astcd { inline namespace ASTC_VARIANT {

struct DecodeVolumeGradRecord {
	DecodeVolumeRecord vol;           // the forward call's record; `out`, `row`, `x_step` and `fmt` are those of grad_out, which is read
	float*   grad_coords;             // point (i, j): grad_coords[j * grad_coord_row + 3 i], dL/du, dL/dv, dL/dw
	size_t   grad_coord_row;          // floats from row to row of points
	float*   grad_lod;                // point (i, j): grad_lod[j * grad_lod_row + i]; null: not wanted
	size_t   grad_lod_row;
};
static_assert(sizeof(DecodeVolumeGradRecord) % 8 == 0, "records are read word by word and hold pointers");

inline size_t decode_volume_grad_levels_offset(uint32_t count) { return decode_lod_levels_offset<DecodeVolumeGradRecord>(count); }
inline size_t decode_volume_grad_bytes(const DecodeLodGradLaunch* grids, uint32_t count) { return decode_lod_table_bytes<DecodeVolumeGradRecord>(grids, count); }

/* The gradient call's table (decode_lod_table_build): the volume call's record and the two buffers that are written. */
inline uint32_t decode_volume_grad_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                         const DecodeLodGradLaunch* grids, uint32_t count)
{
	return decode_lod_table_build<DecodeVolumeGradRecord>(out, images, streams, format, sampler, grids, count, [&](DecodeVolumeGradRecord& r, const DecodeLodGradLaunch& g) -> DecodeVolumeRecord&
	{
		r.grad_coords = g.d_grad_coords;
		r.grad_coord_row = g.grad_coord_row_pitch;
		r.grad_lod = g.d_grad_lod;
		r.grad_lod_row = g.grad_lod_row_pitch;
		r.vol.coords = g.lod.d_coords;
		r.vol.coord_row = g.lod.coord_row_pitch;
		r.vol.address_x = sampler.address_x; r.vol.address_y = sampler.address_y; r.vol.address_z = sampler.address_z;
		return r.vol;
	});
}

/* lod_grad_upstream for a record of the volume family: element `at` (+ c planes, or + c) of grad_out for the format's channels,
 * widened exactly to binary32; the other components are +0.0 and are in no sum. */
template <uint32_t kType, uint32_t kLayout>
WV_FN void volume_grad_upstream(const DecodeVolumeRecord& rec, size_t at, float a[4])
{
	// (lod_grad_upstream reads `out` and `fmt` only: a lod record that holds the two)
	DecodeLodRecord of = {};
	of.out = rec.out;
	of.fmt = rec.fmt;
	lod_grad_upstream<kType, kLayout>(of, at, a);
}

/* volume_axis_taps for a gradient: under BILINEAR both indices of the axis are addressed, whatever their weights. */
__attribute__((always_inline)) WV_FN VolumeAxisTaps volume_grad_axis_taps(const SampleAxis& ax, uint32_t filter, uint32_t mode, uint32_t S, uint32_t block)
{
	const uint32_t taps = filter == 0u ? 1u : 2u;
	VolumeAxisTaps r;
	for (int a = 0; a < 2; a++)
	{
		uint32_t k = 0u;
		r.k[a] = 0xFFFFFFFFu;
		if ((uint32_t)a < taps) r.k[a] = sample_address(mode, ax.i0 + a, S, k) ? k : 0xFFFFFFFFu;
		// (the quotient of a tap that is not there is not used)
		r.b[a] = r.k[a] / block;
		r.t[a] = r.k[a] - r.b[a] * block;
	}
	return r;
}

/* volume_point_taps for a gradient: all eight taps are formed under BILINEAR; P.nx, P.ny, P.nz and the weights stay the forward
 * call's, so sample_point_sums forms the forward sample. */
__attribute__((always_inline)) WV_FN void volume_grad_point_taps(VolumePoint& P, const DecodeImage& img, uint32_t filter, uint32_t address_x, uint32_t address_y,
                                                                 uint32_t address_z, double x, double y, double z)
{
	const SampleAxis ax = sample_axis(filter, x), ay = sample_axis(filter, y), az = sample_axis(filter, z);
	P.nx = ax.n; P.ny = ay.n; P.nz = az.n;
	P.wx[0] = ax.w0; P.wx[1] = ax.w1; P.wy[0] = ay.w0; P.wy[1] = ay.w1; P.wz[0] = az.w0; P.wz[1] = az.w1;
	const VolumeAxisTaps tx = volume_grad_axis_taps(ax, filter, address_x, img.dim_x, img.block_x);
	const VolumeAxisTaps ty = volume_grad_axis_taps(ay, filter, address_y, img.dim_y, img.block_y);
	const VolumeAxisTaps tz = volume_grad_axis_taps(az, filter, address_z, img.dim_z, img.block_z);
#if WV_DEVICE
	#pragma unroll
#endif
	for (int t = 0; t < VOLUME_TAPS; t++)
	{
		const int a = t & 1, b = (t >> 1) & 1, c = t >> 2;
		if (tx.k[a] == 0xFFFFFFFFu || ty.k[b] == 0xFFFFFFFFu || tz.k[c] == 0xFFFFFFFFu) continue;
		P.blk[t] = (tz.b[c] * img.blocks_y + ty.b[b]) * img.blocks_x + tx.b[a];
		P.txyz[t] = tx.t[a] | (ty.t[b] << 8) | (tz.t[c] << 16);
		P.pending |= 1u << t;
	}
}

/* w0 * p0 [+ w1 * p1]: the weighted sum over the forward taps of an axis, which has `n` of them. */
__attribute__((always_inline)) WV_FN double volume_grad_axis_sum(const double w[2], uint32_t n, double p0, double p1)
{
	double r = w[0] * p0;
	if (n > 1u) r = r + w[1] * p1;
	return r;
}

/* What a point keeps of a level: Dx, Dy, Dz and S (d[0 .. 3]) from its decoded taps and the upstream gradient a[c] (binary32,
 * widened here and multiplied by scale[c]: one product).  Every sum starts as its first product.  One channel at a time, so that
 * one channel's eight widened texels are live. */
__attribute__((always_inline)) WV_FN void volume_grad_point_sums(const VolumePoint& P, const TensorParams& fmt, uint32_t filter, const float a[4], uint32_t W, uint32_t H,
                                                                 uint32_t D, double d[4])
{
	float s[4];
	sample_point_sums(P, s);
	double sx = 0.0, sy = 0.0, sz = 0.0, ss = 0.0;
#if WV_DEVICE
	#pragma clang loop unroll(disable)
#endif
	for (int c = 0; c < 4; c++)
	{
		if ((uint32_t)c >= fmt.channels) continue;
		const float ac32 = c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3];
		const float sc32 = c == 0 ? fmt.scale[0] : c == 1 ? fmt.scale[1] : c == 2 ? fmt.scale[2] : fmt.scale[3];
		const float s32 = c == 0 ? s[0] : c == 1 ? s[1] : c == 2 ? s[2] : s[3];
		const double ac = (double)ac32 * (double)sc32;
		const double ps = ac * (double)s32;
		ss = c == 0 ? ps : ss + ps;
		if (filter == 0u) continue;
		// (slot = z tap * 4 + y tap * 2 + x tap)
		double v[VOLUME_TAPS];
		for (int t = 0; t < VOLUME_TAPS; t++) v[t] = (double)(c == 0 ? P.v[t][0] : c == 1 ? P.v[t][1] : c == 2 ? P.v[t][2] : P.v[t][3]);
		const double qx0 = volume_grad_axis_sum(P.wy, P.ny, v[1] - v[0], v[3] - v[2]);
		const double qx1 = volume_grad_axis_sum(P.wy, P.ny, v[5] - v[4], v[7] - v[6]);
		const double dx = volume_grad_axis_sum(P.wz, P.nz, qx0, qx1);
		const double ry0 = volume_grad_axis_sum(P.wx, P.nx, v[2] - v[0], v[3] - v[1]);
		const double ry1 = volume_grad_axis_sum(P.wx, P.nx, v[6] - v[4], v[7] - v[5]);
		const double dy = volume_grad_axis_sum(P.wz, P.nz, ry0, ry1);
		const double rz0 = volume_grad_axis_sum(P.wx, P.nx, v[4] - v[0], v[5] - v[1]);
		const double rz1 = volume_grad_axis_sum(P.wx, P.nx, v[6] - v[2], v[7] - v[3]);
		const double dz = volume_grad_axis_sum(P.wy, P.ny, rz0, rz1);
		const double px = ac * dx, py = ac * dy, pz = ac * dz;
		sx = c == 0 ? px : sx + px;
		sy = c == 0 ? py : sy + py;
		sz = c == 0 ? pz : sz + pz;
	}
	d[0] = filter == 0u ? 0.0 : sx * (double)W;
	d[1] = filter == 0u ? 0.0 : sy * (double)H;
	d[2] = filter == 0u ? 0.0 : sz * (double)D;
	d[3] = ss;
}

/* What a lane keeps of its point across the level passes. */
struct VolumeGradPoint {
	VolumeUVW at;
	uint32_t l0, l1;                  // its levels; l1 = LOD_NO_LEVEL: one level.  l1 may have weight zero (read for S alone)
	double   g;                       // the weight of l1
	double   d0[4], d1[4];            // Dx, Dy, Dz and S of l0 and of l1
	float    a[4];                    // the upstream gradient, widened
	uint32_t live;                    // the lane has a point / the point is valid / lambda' is not clamped under MIP_LINEAR: bits 0 / 1 / 2
};

#if WV_DEVICE
#define VOLUME_GRAD_POINTS_DECL VolumeGradPoint grad_regs
#define VOLUME_GRAD_POINT(l) grad_regs
#else
#define VOLUME_GRAD_POINTS_DECL VolumeGradPoint grad_lanes[SAMPLE_POINTS]
#define VOLUME_GRAD_POINT(l) grad_lanes[l]
#endif

/* Tile `local` of the grid of `grad` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's.  level(l):
 * the DecodeLodLevel of the grid's level l, as in lod_walk_tile.  The counts are lod_walk_tile's, for the harness. */
template <uint32_t kType, uint32_t kLayout, class LevelOf>
WV_FN LodTileCount decode_volume_grad_tile(const DecodeVolumeGradRecord& grad, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	const DecodeVolumeRecord& rec = grad.vol;
	const uint32_t tw_log2 = rec.tw_log2, tw_mask = (1u << tw_log2) - 1u, th_log2 = 6u - tw_log2;
	const uint32_t tile_y = local / rec.tiles_x, tile_x = local - tile_y * rec.tiles_x;
	const uint32_t i0 = tile_x << tw_log2, j0 = tile_y << th_log2;
#if WV_DEVICE
	VolumePoint point_regs;
#else
	VolumePoint point_lanes[SAMPLE_POINTS];
#endif
	VOLUME_GRAD_POINTS_DECL;
	LodTileCount did = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };

	// ---- the levels and the upstream gradient of every point ----
	WV_FOR64(l, 64)
	{
		VolumeGradPoint& Q = VOLUME_GRAD_POINT(l);
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		Q.live = i < rec.out_x && j < rec.out_y ? 1u : 0u;
		Q.at = VolumePoints::none();
		Q.l0 = LOD_NO_LEVEL; Q.l1 = LOD_NO_LEVEL; Q.g = 0.0;
		for (int k = 0; k < 4; k++) { Q.d0[k] = 0.0; Q.d1[k] = 0.0; }
		for (int c = 0; c < 4; c++) Q.a[c] = 0.0f;
		if (Q.live)
		{
			const VolumeUVW at = VolumePoints::read(rec, i, j);
			const float lambda = (rec.lod ? rec.lod[(size_t)j * rec.lod_row + (size_t)i] : 0.0f) + rec.lod_bias;
			if (VolumePoints::valid(at, lambda))
			{
				const LodLevels lv = lod_levels(rec.mip_filter, rec.level_count, lambda);
				// (lambda' in [0, level_count - 1): lambda_c is lambda' and l0 + 1 is a level of the chain)
				const bool slope = rec.mip_filter == 1u && lambda >= 0.0f && lambda < (float)(rec.level_count - 1u);
				Q.live = slope ? 7u : 3u;
				Q.at = at;
				Q.l0 = lv.l0; Q.l1 = lv.l1; Q.g = lv.g;
				if (slope && grad.grad_lod) Q.l1 = lv.l0 + 1u;
				volume_grad_upstream<kType, kLayout>(rec, (size_t)j * rec.row + (size_t)i * rec.x_step, Q.a);
#if !WV_DEVICE
				if (Q.l0 >= rec.level_count || (Q.l1 != LOD_NO_LEVEL && Q.l1 >= rec.level_count)) __builtin_trap();
				if (rec.mip_filter == 1u) { if (lv.l1 != LOD_NO_LEVEL) did.blended = 1u; else did.single = 1u; }
#endif
			}
		}
	}

	// ---- a pass per distinct level, ascending ----
	SampleTileCount done = { 0u, 0u };
	uint32_t lower = 0u;
	for (;;)
	{
		uint32_t m = LOD_NO_LEVEL;
		WV_FOR64(l, 64)
		{
			const VolumeGradPoint& Q = VOLUME_GRAD_POINT(l);
			// (l1 is l0 + 1 or none, and none is the largest value)
			const uint32_t next = Q.l0 >= lower ? Q.l0 : Q.l1;
			if (next >= lower && next < m) m = next;
		}
		m = sample_all_umin(m);
		if (m == LOD_NO_LEVEL) break;
		const DecodeLodLevel lv = level(m);
		WV_FOR64(l, 64)
		{
			VolumePoint& P = SAMPLE_POINT(l);
			const VolumeGradPoint& Q = VOLUME_GRAD_POINT(l);
			P.live = Q.live;
			sample_point_clear(P);
			// (exact products: 24 bits by 17)
			if (Q.l0 == m || Q.l1 == m)
				volume_grad_point_taps(P, lv.img, rec.filter, rec.address_x, rec.address_y, rec.address_z, (double)Q.at.u * (double)lv.img.dim_x,
				                       (double)Q.at.v * (double)lv.img.dim_y, (double)Q.at.w * (double)lv.img.dim_z);
		}
#if !WV_DEVICE
		const uint32_t blocks_before = done.blocks;
#endif
		sample_batches(lv.img, lv.blocks, batch, tile, SAMPLE_POINTS_ARG, done);
#if !WV_DEVICE
		if (done.blocks - blocks_before > did.most) did.most = done.blocks - blocks_before;
#endif
		WV_FOR64(l, 64)
		{
			const VolumePoint& P = SAMPLE_POINT(l);
			VolumeGradPoint& Q = VOLUME_GRAD_POINT(l);
			if (Q.l0 != m && Q.l1 != m) continue;
			double d[4];
			volume_grad_point_sums(P, rec.fmt, rec.filter, Q.a, lv.img.dim_x, lv.img.dim_y, lv.img.dim_z, d);
			for (int k = 0; k < 4; k++)
			{
				Q.d0[k] = Q.l0 == m ? d[k] : Q.d0[k];
				Q.d1[k] = Q.l0 == m ? Q.d1[k] : d[k];
			}
		}
		lower = m + 1u;
		did.passes++;
		did.level_mask |= 1u << m;
	}
	did.batches = done.batches; did.blocks = done.blocks;

	// ---- the blend, one rounding, NaNs canonical; plain vector stores ----
	WV_FOR64(l, 64)
	{
		const VolumeGradPoint& Q = VOLUME_GRAD_POINT(l);
		if (!(Q.live & 1u)) continue;
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		// (an invalid point has kept its +0.0)
		float gc[3] = { (float)Q.d0[0], (float)Q.d0[1], (float)Q.d0[2] }, gl = 0.0f;
		if (Q.g != 0.0)
		{
			const double w0 = 1.0 - Q.g;
			for (int k = 0; k < 3; k++)
			{
				const double p0 = w0 * Q.d0[k], p1 = Q.g * Q.d1[k];
				gc[k] = (float)(p0 + p1);
			}
		}
		if (Q.live & 4u) gl = (float)(Q.d1[3] - Q.d0[3]);
		// (three floats are not 8-byte aligned: three dwords)
		float* at = grad.grad_coords + (size_t)j * grad.grad_coord_row + 3u * (size_t)i;
		for (int k = 0; k < 3; k++)
		{
			const uint32_t bits = tensor_f32_bits<false>(gc[k]);
			__builtin_memcpy(at + k, &bits, 4);
		}
		if (grad.grad_lod)
		{
			const uint32_t bits = tensor_f32_bits<false>(gl);
			__builtin_memcpy(grad.grad_lod + (size_t)j * grad.grad_lod_row + (size_t)i, &bits, 4);
		}
	}
	WV_SYNC();
	return did;
}

} } // namespace astcd::ASTC_VARIANT
