// SPDX-License-Identifier: Apache-2.0
// The gradients of the level-of-detail sampler (astcenc_amd_sample_lod_grad_device): for every point of a grid and an upstream
// gradient of the forward call's output, d loss / d (u, v) and d loss / d lambda -- the vector-Jacobian product of
// astcenc_amd_sample_lod_tensors_device with respect to its coordinates and levels of detail; the texels are compressed and fixed
// (include/astcenc_amd.h has the definition, tests/sample_lod_grad_model.py spells it out in numpy).
//
// A work item is a tile of 64 points of one grid, the tiles and the level walk of decode_lod.h; the lane is the point.  A lane's
// levels are the forward call's and, where grad_lod is wanted and lambda' is not clamped under MIP_LINEAR, level l0 + 1 even when
// its weight is zero: the derivative along lambda is the difference of the two levels' samples.  A level pass is decode_sample.h's
// pipeline with a tap former that keeps all four taps under BILINEAR (the difference along an axis needs both indices of that
// axis even where the forward tap 1 has weight zero); after the batches the lane forms the forward sample (sample_point_sums:
// the taps of weight zero are not in it), the difference sums along x and y and, with the upstream gradient, the three binary64
// values it keeps of the level: Dx, Dy and S.  After the last pass the lane blends (two products and a sum, one rounding) and
// stores the pair with one 8-byte store and the level-of-detail gradient with one 4-byte store.
//
// Included by kernel_decode_lod_grad.hip, decode_volume_grad.h (the launch's table writer and lod_grad_upstream) and
// tests/harness/decode_lod_grad_check.cpp only.
//
// Layout: decode_lod.h's with DecodeLodGradRecord in the place of DecodeLodRecord: ImageSetTable (count = grids, total = tiles),
// first[count], padding, DecodeLodGradRecord[count], then the DecodeLodLevel records of grid 0's levels, of grid 1's ...
#pragma once
#include "decode_lod.h"

namespace astcd { inline namespace ASTC_VARIANT {

struct DecodeLodGradRecord {
	DecodeLodRecord lod;              // the forward call's record; `out`, `row`, `x_step` and `fmt` are those of grad_out, which is read
	float*   grad_coords;             // point (i, j): grad_coords[j * grad_coord_row + 2 i], dL/du then dL/dv
	size_t   grad_coord_row;          // floats from row to row of points
	float*   grad_lod;                // point (i, j): grad_lod[j * grad_lod_row + i]; null: not wanted
	size_t   grad_lod_row;
};
static_assert(sizeof(DecodeLodGradRecord) % 8 == 0, "records are read word by word and hold pointers");

inline size_t decode_lod_grad_levels_offset(uint32_t count) { return decode_lod_levels_offset<DecodeLodGradRecord>(count); }
inline size_t decode_lod_grad_bytes(const DecodeLodGradLaunch* grids, uint32_t count) { return decode_lod_table_bytes<DecodeLodGradRecord>(grids, count); }

/* The gradient call's table (decode_lod_table_build): the forward call's record and the two buffers that are written. */
inline uint32_t decode_lod_grad_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                      const DecodeLodGradLaunch* grids, uint32_t count)
{
	return decode_lod_table_build<DecodeLodGradRecord>(out, images, streams, format, sampler, grids, count, [&](DecodeLodGradRecord& r, const DecodeLodGradLaunch& g) -> DecodeLodRecord&
	{
		r.grad_coords = g.d_grad_coords;
		r.grad_coord_row = g.grad_coord_row_pitch;
		r.grad_lod = g.d_grad_lod;
		r.grad_lod_row = g.grad_lod_row_pitch;
		return decode_lod_own(r.lod, sampler, g.lod);
	});
}

/* Element `at` (+ c planes, or + c) of grad_out for the format's channels, widened exactly to binary32; the other components
 * are +0.0 and are in no sum. */
template <uint32_t kType, uint32_t kLayout>
WV_FN void lod_grad_upstream(const DecodeLodRecord& rec, size_t at, float a[4])
{
	const size_t step = kLayout == 1 ? (size_t)1 : rec.fmt.plane;
	for (int c = 0; c < 4; c++)
	{
		a[c] = 0.0f;
		if ((uint32_t)c >= rec.fmt.channels) continue;
		if (kType == 0)
		{
			a[c] = static_cast<const float*>(rec.out)[at + (size_t)c * step];
			continue;
		}
		const uint16_t h = static_cast<const uint16_t*>(rec.out)[at + (size_t)c * step];
		a[c] = kType == 1 ? tensor_widen_half(h) : int_as_float((int)((uint32_t)h << 16));
	}
}

/* sample_point_taps for a gradient: under BILINEAR both indices of either axis are addressed and all four taps are formed,
 * whatever their weights; P.nx, P.ny and the weights stay the forward call's, so sample_point_sums forms the forward sample. */
__attribute__((always_inline)) WV_FN void lod_grad_point_taps(SamplePoint& P, const DecodeImage& img, uint32_t z, uint32_t filter, uint32_t address_x, uint32_t address_y,
                                                              double x, double y)
{
	const uint32_t block_x = img.block_x, block_y = img.block_y;
	const SampleAxis ax = sample_axis(filter, x), ay = sample_axis(filter, y);
	P.nx = ax.n; P.ny = ay.n;
	P.wx[0] = ax.w0; P.wx[1] = ax.w1; P.wy[0] = ay.w0; P.wy[1] = ay.w1;
	const uint32_t taps = filter == 0u ? 1u : 2u;
	uint32_t kx[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu }, ky[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu };
	for (int a = 0; a < 2; a++)
	{
		if ((uint32_t)a >= taps) continue;
		uint32_t k = 0u;
		kx[a] = sample_address(address_x, ax.i0 + a, img.dim_x, k) ? k : 0xFFFFFFFFu;
		ky[a] = sample_address(address_y, ay.i0 + a, img.dim_y, k) ? k : 0xFFFFFFFFu;
	}
	const uint32_t bx[2] = { kx[0] / block_x, kx[1] / block_x }, by[2] = { ky[0] / block_y, ky[1] / block_y };
#if WV_DEVICE
	#pragma unroll
#endif
	for (int t = 0; t < SAMPLE_TAPS; t++)
	{
		if (kx[t & 1] == 0xFFFFFFFFu || ky[t >> 1] == 0xFFFFFFFFu) continue;
		P.blk[t] = (z * img.blocks_y + by[t >> 1]) * img.blocks_x + bx[t & 1];
		P.txy[t] = (kx[t & 1] - bx[t & 1] * block_x) | ((ky[t >> 1] - by[t >> 1] * block_y) << 8);
		P.pending |= 1u << t;
	}
}

/* What a point keeps of a level: Dx, Dy and S (d[0 .. 2]) from its decoded taps and the upstream gradient a[c] (binary32,
 * widened here and multiplied by scale[c]: one product).  Every sum starts as its first product. */
__attribute__((always_inline)) WV_FN void lod_grad_point_sums(const SamplePoint& P, const TensorParams& fmt, uint32_t filter, const float a[4], uint32_t W, uint32_t H,
                                                              double d[3])
{
	float s[4];
	sample_point_sums(P, s);
	double sx = 0.0, sy = 0.0, ss = 0.0;
	for (int c = 0; c < 4; c++)
	{
		if ((uint32_t)c >= fmt.channels) continue;
		const double ac = (double)a[c] * (double)fmt.scale[c];
		const double ps = ac * (double)s[c];
		ss = c == 0 ? ps : ss + ps;
		if (filter == 0u) continue;
		const double v00 = (double)P.v[0][c], v10 = (double)P.v[1][c], v01 = (double)P.v[2][c], v11 = (double)P.v[3][c];
		double dx = P.wy[0] * (v10 - v00);
		if (P.ny > 1u) dx = dx + P.wy[1] * (v11 - v01);
		double dy = P.wx[0] * (v01 - v00);
		if (P.nx > 1u) dy = dy + P.wx[1] * (v11 - v10);
		const double px = ac * dx, py = ac * dy;
		sx = c == 0 ? px : sx + px;
		sy = c == 0 ? py : sy + py;
	}
	d[0] = filter == 0u ? 0.0 : sx * (double)W;
	d[1] = filter == 0u ? 0.0 : sy * (double)H;
	d[2] = ss;
}

/* What a lane keeps of its point across the level passes. */
struct LodGradPoint {
	LodUV    at;
	uint32_t l0, l1;                  // its levels; l1 = LOD_NO_LEVEL: one level.  l1 may have weight zero (read for S alone)
	double   g;                       // the weight of l1
	double   d0[3], d1[3];            // Dx, Dy and S of l0 and of l1
	float    a[4];                    // the upstream gradient, widened
	uint32_t live;                    // the lane has a point / the point is valid / lambda' is not clamped under MIP_LINEAR: bits 0 / 1 / 2
};

#if WV_DEVICE
#define LOD_GRAD_POINTS_DECL LodGradPoint grad_regs
#define LOD_GRAD_POINT(l) grad_regs
#else
#define LOD_GRAD_POINTS_DECL LodGradPoint grad_lanes[SAMPLE_POINTS]
#define LOD_GRAD_POINT(l) grad_lanes[l]
#endif

/* Tile `local` of the grid of `rec` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's.  level(l):
 * the DecodeLodLevel of the grid's level l, as in lod_walk_tile.  The counts are lod_walk_tile's, for the harness. */
template <uint32_t kType, uint32_t kLayout, class LevelOf>
WV_FN LodTileCount decode_lod_grad_tile(const DecodeLodGradRecord& grad, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	const DecodeLodRecord& rec = grad.lod;
	const uint32_t tw_log2 = rec.tw_log2, tw_mask = (1u << tw_log2) - 1u, th_log2 = 6u - tw_log2;
	const uint32_t tile_y = local / rec.tiles_x, tile_x = local - tile_y * rec.tiles_x;
	const uint32_t i0 = tile_x << tw_log2, j0 = tile_y << th_log2;
	SAMPLE_POINTS_DECL;
	LOD_GRAD_POINTS_DECL;
	LodTileCount did = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };

	// ---- the levels and the upstream gradient of every point ----
	WV_FOR64(l, 64)
	{
		LodGradPoint& Q = LOD_GRAD_POINT(l);
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		Q.live = i < rec.out_x && j < rec.out_y ? 1u : 0u;
		Q.at = LodUVPoints::none();
		Q.l0 = LOD_NO_LEVEL; Q.l1 = LOD_NO_LEVEL; Q.g = 0.0;
		for (int k = 0; k < 3; k++) { Q.d0[k] = 0.0; Q.d1[k] = 0.0; }
		for (int c = 0; c < 4; c++) Q.a[c] = 0.0f;
		if (Q.live)
		{
			const LodUV at = LodUVPoints::read(rec, i, j);
			const float lambda = (rec.lod ? rec.lod[(size_t)j * rec.lod_row + (size_t)i] : 0.0f) + rec.lod_bias;
			if (LodUVPoints::valid(at, lambda))
			{
				const LodLevels lv = lod_levels(rec.mip_filter, rec.level_count, lambda);
				// (lambda' in [0, level_count - 1): lambda_c is lambda' and l0 + 1 is a level of the chain)
				const bool slope = rec.mip_filter == 1u && lambda >= 0.0f && lambda < (float)(rec.level_count - 1u);
				Q.live = slope ? 7u : 3u;
				Q.at = at;
				Q.l0 = lv.l0; Q.l1 = lv.l1; Q.g = lv.g;
				if (slope && grad.grad_lod) Q.l1 = lv.l0 + 1u;
				lod_grad_upstream<kType, kLayout>(rec, (size_t)j * rec.row + (size_t)i * rec.x_step, Q.a);
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
			const LodGradPoint& Q = LOD_GRAD_POINT(l);
			// (l1 is l0 + 1 or none, and none is the largest value)
			const uint32_t next = Q.l0 >= lower ? Q.l0 : Q.l1;
			if (next >= lower && next < m) m = next;
		}
		m = sample_all_umin(m);
		if (m == LOD_NO_LEVEL) break;
		const DecodeLodLevel lv = level(m);
		WV_FOR64(l, 64)
		{
			SamplePoint& P = SAMPLE_POINT(l);
			const LodGradPoint& Q = LOD_GRAD_POINT(l);
			P.live = Q.live;
			sample_point_clear(P);
			// (exact products: 24 bits by 17)
			if (Q.l0 == m || Q.l1 == m)
				lod_grad_point_taps(P, lv.img, rec.z, rec.filter, rec.address_x, rec.address_y, (double)Q.at.u * (double)lv.img.dim_x, (double)Q.at.v * (double)lv.img.dim_y);
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
			const SamplePoint& P = SAMPLE_POINT(l);
			LodGradPoint& Q = LOD_GRAD_POINT(l);
			if (Q.l0 != m && Q.l1 != m) continue;
			double d[3];
			lod_grad_point_sums(P, rec.fmt, rec.filter, Q.a, lv.img.dim_x, lv.img.dim_y, d);
			for (int k = 0; k < 3; k++)
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
		const LodGradPoint& Q = LOD_GRAD_POINT(l);
		if (!(Q.live & 1u)) continue;
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		// (an invalid point has kept its +0.0)
		float gu = (float)Q.d0[0], gv = (float)Q.d0[1], gl = 0.0f;
		if (Q.g != 0.0)
		{
			const double w0 = 1.0 - Q.g;
			const double pu0 = w0 * Q.d0[0], pu1 = Q.g * Q.d1[0], pv0 = w0 * Q.d0[1], pv1 = Q.g * Q.d1[1];
			gu = (float)(pu0 + pu1);
			gv = (float)(pv0 + pv1);
		}
		if (Q.live & 4u) gl = (float)(Q.d1[2] - Q.d0[2]);
		// (grad_coords is aligned to 8 bytes and the pitch is even: one 8-byte store)
		const uint32_t pair[2] = { tensor_f32_bits<false>(gu), tensor_f32_bits<false>(gv) };
		__builtin_memcpy(__builtin_assume_aligned(grad.grad_coords + (size_t)j * grad.grad_coord_row + 2u * (size_t)i, 8), pair, 8);
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
