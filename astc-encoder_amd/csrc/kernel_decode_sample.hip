// SPDX-License-Identifier: Apache-2.0
// Compressed images sampled at coordinates into tensors (astcenc_amd_sample_tensors_device): one wavefront per tile of 64 points
// of a grid, the lane is the point; the wave decodes the distinct blocks its points' taps reach in batches, through the
// decoder's own phases and per-texel body, and every lane blends its taps in registers (decode_sample.h).  A translation unit
// of its own, so that kernel_decode.hip and kernel_decode_scaled.hip and their kernels are what they were.
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_sample.h"
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <vector>

namespace astcd {

// LDS of a workgroup: DecodeBatch and the batch's block list, nothing else.
static_assert(sizeof(DecodeBatch) == 7040 && sizeof(SampleTile) == 4 * DECODE_BATCH, "astc_decode_sample: DecodeBatch (7040 B) and the list of a batch's blocks (128 B)");

/* The tiles of every grid back to back on a 1D grid, a tile's grid found in the table (image_set.h).  `tile0`: the launch covers
 * tiles [tile0, tile0 + gridDim.x) of the call.  One build per tensor type and layout, which hold for a call; filter, address
 * modes and the entry's data type are wave-uniform values of the record. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64)
astc_decode_sample(const ImageSetTable* __restrict__ set, uint32_t tile0)
{
	__shared__ DecodeBatch batch;
	__shared__ SampleTile tile;
	typedef const __attribute__((address_space(4))) uint8_t* constant_bytes;
	const constant_bytes t = (constant_bytes)reinterpret_cast<uintptr_t>(set);
	const uint32_t count = reinterpret_cast<const __attribute__((address_space(4))) ImageSetTable*>(t)->count;
	const __attribute__((address_space(4))) uint32_t* first = reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(t + image_set_first_offset());
	const uint32_t r = tile0 + blockIdx.x;
	const uint32_t g = image_set_find(first, count, r);
	const DecodeSampleRecord rec = image_set_record<DecodeSampleRecord>(reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(
		t + image_set_records_offset(count) + (size_t)g * sizeof(DecodeSampleRecord)));
	(void)decode_sample_tile<kType, kLayout>(rec, r - first[g], batch, tile);
}

unsigned long long astc_decode_sample_tiles(uint32_t out_x, uint32_t out_y) { return decode_sample_tiles(out_x, out_y); }

size_t astc_decode_sample_bytes(uint32_t count) { return decode_sample_bytes(count); }

uint32_t astc_decode_sample_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeSampler& sampler,
                                  const DecodeSampleLaunch* grids, uint32_t count)
{
	std::vector<DecodeImage> images(entry_count);
	std::vector<const uint8_t*> streams(entry_count);
	for (uint32_t e = 0; e < entry_count; e++)
	{
		images[e] = decode_sample_image(entries[e]);
		streams[e] = entries[e].d_blocks;
	}
	return decode_sample_build(out, images.data(), streams.data(), format, sampler, grids, count);
}

int astc_decode_sample_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	typedef void (*Kernel)(const ImageSetTable*, uint32_t);
	static const Kernel kernels[3][2] = { { astc_decode_sample<0, 0>, astc_decode_sample<0, 1> }, { astc_decode_sample<1, 0>, astc_decode_sample<1, 1> },
	                                      { astc_decode_sample<2, 0>, astc_decode_sample<2, 1> } };
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
