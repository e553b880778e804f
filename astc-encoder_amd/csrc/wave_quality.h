// SPDX-License-Identifier: Apache-2.0
// Quality of compressed blocks against the source image without a decoded image in memory: the batched decoder
// (wave_decode.h, decode_row_batch) with a texel sink that, where the decoder stores a texel, loads the original's texel at the
// same place and accumulates the error terms of the quality report (wave_metrics.h).
//   ref: compute_error_metrics   Source/astcenccli_error_metrics.cpp:110-300
// The decoded operand is formed from the bits the decoder would have stored -- the packed RGBA8 pixel read through the unorm8
// table, the half read back through half_to_float, the float -- with the operand clamp of metric_load_texel, so every
// per-texel term is the one astc_compare_images forms over the decoded image.  Sums are fp64 and added in a fixed order:
//   a lane adds the terms of its texels in the order the texel phase visits them (2D: its column's rows top to bottom, trip
//   after trip; 3D: its texels of the run in index order);
//   per block (on request): after every trip of 64 elements the lanes' sums of that trip go through LDS and the block's lane
//   adds those of its elements in element order;
//   per run: a shuffle tree over the 64 lanes (lane l takes lane l + 32, then + 16, ... + 1).
#pragma once
#include "wave_decode.h"
#include "wave_metrics.h"

namespace astcd { inline namespace ASTC_VARIANT {

/* N values per lane, declared outside the WV_FOR loops and used inside them with the loop's lane: registers on the device,
 * an array in the sequential build. */
template <typename T, int N>
struct PerLane {
#if WV_DEVICE
	T v[N];
	WV_FN T& at(int, int i) { return v[i]; }
	WV_FN void fill(T x) { for (int i = 0; i < N; i++) v[i] = x; }
#else
	T v[64][N];
	WV_FN T& at(int lane, int i) { return v[lane][i]; }
	WV_FN void fill(T x) { for (int l = 0; l < 64; l++) for (int i = 0; i < N; i++) v[l][i] = x; }
#endif
};

/* Per-wave scratch (LDS) next to the decoder's DecodeBatch. */
struct alignas(16) QualityScratch {
	double stage[64][4];     // the lanes' squared-error sums of one trip, on their way to the blocks' lanes
	float  unorm8[256];      // (float)i / 255.0f, the table of astc_compare_images
};

/* Slots of a run's partial sums: the layout of the totals (wave_metrics.h). */
constexpr int QUALITY_PEAK = 8;

template <bool HDR>
struct QualitySink {
	static constexpr int NACC = HDR ? 16 : 8;
	const void* original;      // image 1 of the comparison: tightly packed RGBA texels of original_type, the decoded image's dimensions
	uint32_t original_type;
	int fstop_lo, fstop_hi;
	bool per_block;
	QualityScratch* q;
	PerLane<double, NACC> acc; // the run: [0..3] squared error, [4..7] alpha-scaled, HDR [8..11] log2, [12..15] mPSNR
	PerLane<float, 1> peak;
	PerLane<double, 4> trip;   // squared error of the lane's texels of the current trip
	PerLane<double, 4> block;  // lane k: squared error of block k of the run
#if !WV_DEVICE
	float* trace;              // sequential build: the terms of every texel (8, HDR 16 floats at texel * NACC), or null
#endif

	WV_FN void begin(const void* image, uint32_t type, int lo, int hi, bool blocks, QualityScratch* scratch)
	{
		original = image; original_type = type; fstop_lo = lo; fstop_hi = hi; per_block = blocks; q = scratch;
		acc.fill(0.0); peak.fill(0.0f); trip.fill(0.0); block.fill(0.0);
#if !WV_DEVICE
		trace = nullptr;
#endif
	}

	/* c2: the decoded texel as metric_load_texel reads it from the decoded image. */
	WV_FN void compare(int lane, size_t at, const float c2[4])
	{
		float c1[4], e[8];
		metric_load_texel(original, at >> 2, original_type, q->unorm8, c1);
		const float m = metric_terms_of(c1, c2, e);
		peak.at(lane, 0) = m > peak.at(lane, 0) ? m : peak.at(lane, 0);
		for (int k = 0; k < 8; k++) acc.at(lane, k) += (double)e[k];
		if (per_block) for (int k = 0; k < 4; k++) trip.at(lane, k) += (double)e[k];
#if !WV_DEVICE
		if (trace) for (int k = 0; k < 8; k++) trace[(at >> 2) * NACC + k] = e[k];
#endif
		if (HDR)
		{
			float h[8];
			metric_hdr_terms(c1, c2, fstop_lo, fstop_hi, h);
			for (int k = 0; k < 8; k++) acc.at(lane, (HDR ? 8 : 0) + k) += (double)h[k];
#if !WV_DEVICE
			if (trace) for (int k = 0; k < 8; k++) trace[(at >> 2) * NACC + (HDR ? 8 : 0) + k] = h[k];
#endif
		}
	}

	// (the three forms of DecodeStore)
	WV_FN void pixel(const DecodeImage&, int lane, size_t at, uint32_t px)
	{
		float c2[4];
		metric_unpack_rgba8(px, q->unorm8, c2);
		compare(lane, at, c2);
	}
	WV_FN void halves(const DecodeImage&, int lane, size_t at, uint64_t px)
	{
		float c2[4];
		for (int k = 0; k < 4; k++) c2[k] = metric_clamp_operand(half_to_float((uint16_t)(px >> (16 * k))));
		compare(lane, at, c2);
	}
	WV_FN void texel(const DecodeImage& img, int lane, size_t at, float r, float g, float b, float a)
	{
		// (what store_texel_at writes, read back)
		float c2[4];
		if (img.data_type == 0) metric_unpack_rgba8(pack_texel_u8(img, r, g, b, a), q->unorm8, c2);
		else
		{
			float src[7];
			swizzle_sources(r, g, b, a, src);
			for (int k = 0; k < 4; k++)
			{
				const float v = src[img.swz[k]];
				c2[k] = metric_clamp_operand(img.data_type == 1 ? half_to_float(float_to_half(v)) : v);
			}
		}
		compare(lane, at, c2);
	}

	/* Elements [base, base + 64) of the run are done (an element: a column of the 2D texel phase, a texel of the 3D one; block
	 * k of the run has elements [k * unit, (k + 1) * unit)): every lane hands its sums of the trip to its element's block. */
	WV_FN void trip_end(int base, int unit, int count)
	{
		if (!per_block) return;
		WV_FOR64(l, 64)
		{
			for (int c = 0; c < 4; c++) { q->stage[l][c] = trip.at(l, c); trip.at(l, c) = 0.0; }
		}
		WV_SYNC();
		WV_FOR64(k, count)
		{
			const int lo = i_max(mul24(k, unit), base) - base, hi = i_min(mul24(k + 1, unit), base + 64) - base;
			for (int i = lo; i < hi; i++)
				for (int c = 0; c < 4; c++) block.at(k, c) += q->stage[i][c];
		}
		WV_SYNC();
	}

	/* The run's sums on lane 0 (acc, peak): the fixed tree over the lanes. */
	WV_FN void fold_run()
	{
#if WV_DEVICE
		for (int off = 32; off > 0; off >>= 1)
		{
			for (int k = 0; k < NACC; k++) acc.v[k] += __shfl_down(acc.v[k], off);
			const float o = __shfl_down(peak.v[0], off);
			peak.v[0] = o > peak.v[0] ? o : peak.v[0];
		}
#else
		for (int off = 32; off > 0; off >>= 1)
			for (int l = 0; l < off; l++)
			{
				for (int k = 0; k < NACC; k++) acc.v[l][k] += acc.v[l + off][k];
				peak.v[l][0] = peak.v[l + off][0] > peak.v[l][0] ? peak.v[l + off][0] : peak.v[l][0];
			}
#endif
	}
};

/* What decode_row_batch does for blocks bx0 .. bx0 + count - 1 of block row `by`, layer `bz`, with the comparison in place of
 * the stores (img.data is not used).  All 64 lanes call this.
 * block_errors: null, or four doubles per block of the stream (raster block order): the squared error of the block's texels
 * inside the image.  partial: the run's sums, quantity i -- the index of the totals, wave_metrics.h -- at partial[i * stride].
 * `sink`: the caller's (the sequential build sets its trace between begin() and here); q: filled here. */
template <bool HDR>
WV_FN void quality_row_batch(const DecodeImage& img, const uint8_t* blocks, uint32_t bx0, uint32_t by, uint32_t bz, int count, DecodeBatch& s,
                             QualitySink<HDR>& sink, double* block_errors, double* partial, size_t stride)
{
	WV_FOR(i, 256) sink.q->unorm8[i] = (float)i / 255.0f;
	WV_SYNC();
	decode_row_batch(img, blocks, bx0, by, bz, count, s, sink);
	if (block_errors)
	{
		const size_t first = ((size_t)bz * img.blocks_y + by) * img.blocks_x + bx0;
		WV_FOR64(k, count)
		{
			double* o = block_errors + (first + (size_t)k) * 4;
			for (int c = 0; c < 4; c++) o[c] = sink.block.at(k, c);
		}
	}
	sink.fold_run();
	WV_ONE
	{
		for (int k = 0; k < 8; k++) partial[(size_t)k * stride] = sink.acc.at(0, k);
		partial[(size_t)QUALITY_PEAK * stride] = (double)sink.peak.at(0, 0);
		if (HDR) for (int k = 0; k < 8; k++) partial[(size_t)(METRIC_HDR_FIRST + k) * stride] = sink.acc.at(0, (HDR ? 8 : 0) + k);
	}
}

} } // namespace astcd::ASTC_VARIANT
