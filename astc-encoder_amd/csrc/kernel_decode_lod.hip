// SPDX-License-Identifier: Apache-2.0
// Compressed mip chains sampled at a level of detail per point (astcenc_amd_sample_lod_tensors_device): one wavefront per tile of
// 64 points of a grid, the lane is the point; the wave walks the distinct mip levels its points need and runs the coordinate
// sampler's pipeline once per level -- taps, batches of distinct blocks through the decoder's own phases, the sums -- then every
// lane blends its one or two levels in registers (decode_lod.h).  A translation unit of its own, so that kernel_decode_sample.hip
// and its kernels are what they were.
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_lod.h"
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <vector>

namespace astcd {

// LDS of a workgroup: what astc_decode_sample has -- DecodeBatch and the batch's block list, nothing else.
static_assert(sizeof(DecodeBatch) + sizeof(SampleTile) == 7168, "astc_lod_sample: DecodeBatch (7040 B) and the list of a batch's blocks (128 B)");

typedef const __attribute__((address_space(4))) uint8_t* lod_constant_bytes;
typedef const __attribute__((address_space(4))) uint32_t* lod_constant_words;

/* The level records of a grid in the table: level l (uniform) read word by word with scalar loads. */
struct LodLevelsOfGrid {
	lod_constant_bytes at;
	__device__ DecodeLodLevel operator()(uint32_t l) const
	{
		return image_set_record<DecodeLodLevel>(reinterpret_cast<lod_constant_words>(at + (size_t)l * sizeof(DecodeLodLevel)));
	}
};

/* The tiles of every grid back to back on a 1D grid, a tile's grid found in the table (image_set.h).  `tile0`: the launch covers
 * tiles [tile0, tile0 + gridDim.x) of the call.  One build per tensor type and layout, which hold for a call; the filters, the
 * address modes and every level's data type are wave-uniform values of the records. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64)
astc_lod_sample(const ImageSetTable* __restrict__ set, uint32_t tile0)
{
	__shared__ DecodeBatch batch;
	__shared__ SampleTile tile;
	const lod_constant_bytes t = (lod_constant_bytes)reinterpret_cast<uintptr_t>(set);
	const uint32_t count = reinterpret_cast<const __attribute__((address_space(4))) ImageSetTable*>(t)->count;
	const lod_constant_words first = reinterpret_cast<lod_constant_words>(t + image_set_first_offset());
	const uint32_t r = tile0 + blockIdx.x;
	const uint32_t g = image_set_find(first, count, r);
	const DecodeLodRecord rec = image_set_record<DecodeLodRecord>(reinterpret_cast<lod_constant_words>(
		t + image_set_records_offset(count) + (size_t)g * sizeof(DecodeLodRecord)));
	const LodLevelsOfGrid levels = { t + rec.levels };
	(void)decode_lod_tile<kType, kLayout>(rec, levels, r - first[g], batch, tile);
}

size_t astc_decode_lod_bytes(const DecodeLodLaunch* grids, uint32_t count) { return decode_lod_bytes(grids, count); }

uint32_t astc_decode_lod_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                               const DecodeLodLaunch* grids, uint32_t count)
{
	std::vector<DecodeImage> images(entry_count);
	std::vector<const uint8_t*> streams(entry_count);
	for (uint32_t e = 0; e < entry_count; e++)
	{
		images[e] = decode_sample_image(entries[e]);
		streams[e] = entries[e].d_blocks;
	}
	return decode_lod_build(out, images.data(), streams.data(), format, sampler, grids, count);
}

int astc_decode_lod_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	typedef void (*Kernel)(const ImageSetTable*, uint32_t);
	static const Kernel kernels[3][2] = { { astc_lod_sample<0, 0>, astc_lod_sample<0, 1> }, { astc_lod_sample<1, 0>, astc_lod_sample<1, 1> },
	                                      { astc_lod_sample<2, 0>, astc_lod_sample<2, 1> } };
	if (type > 2 || layout > 1) return (int)hipErrorInvalidValue;
	// (the grid of astc_decode_set_launch, and its test limit ASTCENC_AMD_DECODE_GRID_LIMIT)
	static const uint32_t limit = []()
	{
		const char* e = getenv("ASTCENC_AMD_DECODE_GRID_LIMIT");
		const long v = e ? strtol(e, nullptr, 10) : 0;
		return v >= 1 && v < 65535 ? (uint32_t)v : 0xFFFFFFFFu / 64u;
	}();
	const ImageSetTable* set = static_cast<const ImageSetTable*>(d_table);
	for (uint32_t tile0 = 0; tile0 < tiles; tile0 += limit)
	{
		const uint32_t n = tiles - tile0 < limit ? tiles - tile0 : limit;
		hipLaunchKernelGGL(kernels[type][layout], dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), set, tile0);
	}
	return (int)hipGetLastError();
}

} // namespace astcd
