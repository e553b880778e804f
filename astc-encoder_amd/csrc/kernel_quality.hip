// SPDX-License-Identifier: Apache-2.0
// Block quality kernel: the error sums of compressed blocks against the source image in one pass, with no decoded image in
// memory (astcenc_amd_compare_blocks_device / _hdr_device / astcenc_amd_compare_image_set_device).  One wavefront per run of
// DECODE_BATCH consecutive blocks of a block row, as in kernel_decode.hip; where the decoder stores a texel the sink of
// wave_quality.h loads the original's and accumulates the terms of astc_compare_images.  Every image is a set (image_set.h):
// the single-image calls are sets of one entry, so an entry's sums are the same doubles alone and in any set.  A set of one
// entry needs no table in device memory: its record travels as a kernel argument (`set` is then null).
//
// Reduction, all of it in a fixed order and without atomics: a run's sums (wave_quality.h) go to the run's slot of the
// partials; astc_quality_finish then adds the slots of each entry -- lane l those of the entry's runs l, l + 64, ... in index
// order, then the shuffle tree over the lanes -- into the entry's totals.  The partials hold QUALITY_MAX_RUNS slots: a launch
// covers consecutive runs up to that many, cut only where an entry ends or at a multiple of QUALITY_MAX_RUNS runs from an
// entry's first run (a piece); the finish pass of a later piece adds to the totals the earlier pieces left.  Where the pieces
// end depends on the entry alone, never on its place in a set.
#define ASTC_VARIANT v_quality
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_quality.h"
#include "decode_kernels.h"

namespace astcd {

constexpr uint32_t QUALITY_MAX_RUNS = 65536;      // slots of the partials: 18 quantities x 8 bytes each, 9 MiB in all
constexpr int QUALITY_FINISH_LOADS = 16;          // independent loads in flight per lane of the finish pass

struct QualitySetEntry {
	DecodeImage img;          // (data unused: nothing is stored)
	const uint8_t* blocks;
	const void* original;
	double* block_errors;     // null, or four doubles per block of the entry
	uint32_t original_type;
	uint32_t runs_x;          // runs per block row: ceil(blocks_x / DECODE_BATCH)
	uint32_t runs_xy;         // ... per layer of blocks
	uint32_t pad;
};

/* Run run0 + blockIdx.x of the set; its sums go to slot blockIdx.x of the partials (quantity i at partials[i * stride + slot]).
 * set == null: the set is the one entry `one`. */
template <bool HDR>
__global__ void __launch_bounds__(64)
astc_quality_set(const ImageSetTable* __restrict__ set, QualitySetEntry one, uint32_t run0, int fstop_lo, int fstop_hi, double* __restrict__ partials, uint32_t stride)
{
	__shared__ DecodeBatch batch;
	__shared__ QualityScratch scratch;
	const uint32_t r = run0 + blockIdx.x;
	QualitySetEntry rec = one;
	uint32_t local = r;
	if (set) rec = decode_table_item<QualitySetEntry>(set, r, local);
	const uint32_t bz = local / rec.runs_xy;
	const uint32_t in_layer = local - bz * rec.runs_xy;
	const uint32_t by = in_layer / rec.runs_x;
	const uint32_t bx0 = (in_layer - by * rec.runs_x) * (uint32_t)DECODE_BATCH;
	const uint32_t left = rec.img.blocks_x - bx0;
	QualitySink<HDR> sink;
	sink.begin(rec.original, rec.original_type, fstop_lo, fstop_hi, rec.block_errors != nullptr, &scratch);
	quality_row_batch<HDR>(rec.img, rec.blocks, bx0, by, bz, (int)(left < (uint32_t)DECODE_BATCH ? left : (uint32_t)DECODE_BATCH), batch, sink,
	                       rec.block_errors, partials + blockIdx.x, (size_t)stride);
}

/* The launch covered runs [run0, run0 + n) of the set; workgroup (x, y): quantity y of entry e0 + x, every one of which has a
 * piece in that range.  sums: METRIC_SUMS_HDR doubles per entry.  set == null: one entry of `total` runs. */
__global__ void __launch_bounds__(64)
astc_quality_finish(const ImageSetTable* __restrict__ set, uint32_t total, uint32_t e0, uint32_t run0, uint32_t n, const double* __restrict__ partials,
                    uint32_t stride, int hdr, double* __restrict__ sums)
{
	const int k = (int)blockIdx.y;
	if (k >= (hdr ? METRIC_SUMS_HDR : 9) || k == 9) return;
	const bool is_peak = k == QUALITY_PEAK;
	const uint32_t e = e0 + blockIdx.x;
	uint32_t begin = 0, end = total;
	if (set)
	{
		const uint32_t* first = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(set) + image_set_first_offset());
		begin = first[e];
		end = e + 1 < set->count ? first[e + 1] : set->total;
	}
	const uint32_t a = begin > run0 ? begin : run0, b = end < run0 + n ? end : run0 + n;
	const double* src = partials + (size_t)k * stride + (a - run0);
	const uint32_t cnt = b - a;
	double v = 0.0;                                         // (every quantity is a sum of squares or a peak of non-negative values)
	for (uint32_t i0 = threadIdx.x; i0 < cnt; i0 += 64u * QUALITY_FINISH_LOADS)
	{
		double p[QUALITY_FINISH_LOADS];
		#pragma unroll
		for (int u = 0; u < QUALITY_FINISH_LOADS; u++)
		{
			const uint32_t i = i0 + 64u * (uint32_t)u;
			p[u] = i < cnt ? src[i] : 0.0;                   // (x + 0 == x, max(x, 0) == x)
		}
		#pragma unroll
		for (int u = 0; u < QUALITY_FINISH_LOADS; u++) v = !is_peak ? v + p[u] : (p[u] > v ? p[u] : v);
	}
	for (int off = 32; off > 0; off >>= 1)
	{
		const double o = __shfl_down(v, off);
		v = !is_peak ? v + o : (o > v ? o : v);
	}
	if (threadIdx.x == 0)
	{
		double* dst = sums + (size_t)e * METRIC_SUMS_HDR + k;
		if (a != begin)                                     // a later piece of the entry: on top of what the earlier ones left
		{
			const double old = *dst;
			v = !is_peak ? old + v : (old > v ? old : v);
		}
		*dst = v;
	}
}

size_t astc_quality_set_bytes(uint32_t count) { return decode_table_bytes<QualitySetEntry>(count); }

size_t astc_quality_scratch_doubles() { return (size_t)QUALITY_MAX_RUNS * METRIC_SUMS_HDR; }

uint32_t astc_quality_set_build(void* out, const QualityLaunch* entries, uint32_t count)
{
	uint32_t* first;
	QualitySetEntry* rec = decode_table_begin<QualitySetEntry>(out, astc_quality_set_bytes(count), count, first);
	uint32_t runs = 0;
	for (uint32_t e = 0; e < count; e++)
	{
		const DecodeLaunch& d = entries[e].decode;
		const DecodeImage& img = rec[e].img = decode_image_of(d, nullptr);
		rec[e].blocks = d.d_blocks;
		rec[e].original = entries[e].d_original;
		rec[e].original_type = entries[e].original_type;
		rec[e].block_errors = entries[e].d_block_errors;
		rec[e].runs_x = (img.blocks_x + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH;
		rec[e].runs_xy = rec[e].runs_x * img.blocks_y;
		first[e] = runs;
		runs += rec[e].runs_xy * img.blocks_z;
	}
	return decode_table_finish(out, count, runs);
}

int astc_quality_set_launch(const void* h_table, const void* d_table, double* d_partials, double* d_sums, int hdr, int fstop_lo, int fstop_hi, void* stream)
{
	// (the decoder's test limit on a launch is the limit on a piece here; the loop below cuts its launches where entries and
	//  pieces end and queues a finish pass behind each, so it is not decode_table_launch's)
	static const uint32_t piece_runs = decode_grid_limit(QUALITY_MAX_RUNS, (long)QUALITY_MAX_RUNS);
	const ImageSetTable* h = static_cast<const ImageSetTable*>(h_table);
	const uint32_t* first = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(h_table) + image_set_first_offset());
	const ImageSetTable* set = static_cast<const ImageSetTable*>(d_table);       // (null for a set of one entry)
	const QualitySetEntry& one = *reinterpret_cast<const QualitySetEntry*>(static_cast<const uint8_t*>(h_table) + image_set_records_offset(h->count));
	const hipStream_t s = static_cast<hipStream_t>(stream);
	const uint32_t count = h->count, total = h->total;
	uint32_t run0 = 0, e = 0;                  // the next launch starts at run0, a piece boundary inside entry e
	while (run0 < total)
	{
		const uint32_t e0 = e;
		uint32_t end = run0, e_last = e;
		while (end < total)
		{
			const uint32_t e_end = e + 1 < count ? first[e + 1] : total;
			const uint32_t piece = e_end - end < piece_runs ? e_end - end : piece_runs;
			if (end != run0 && (end - run0) + piece > piece_runs) break;
			e_last = e;
			end += piece;
			if (end == e_end) e++;
		}
		const uint32_t n = end - run0;
		if (hdr) hipLaunchKernelGGL(astc_quality_set<true>, dim3(n), dim3(64), 0, s, set, one, run0, fstop_lo, fstop_hi, d_partials, QUALITY_MAX_RUNS);
		else hipLaunchKernelGGL(astc_quality_set<false>, dim3(n), dim3(64), 0, s, set, one, run0, 0, 0, d_partials, QUALITY_MAX_RUNS);
		hipLaunchKernelGGL(astc_quality_finish, dim3(e_last - e0 + 1, METRIC_SUMS_HDR), dim3(64), 0, s, set, total, e0, run0, n, d_partials, QUALITY_MAX_RUNS, hdr, d_sums);
		run0 = end;
	}
	return (int)hipGetLastError();
}

} // namespace astcd
