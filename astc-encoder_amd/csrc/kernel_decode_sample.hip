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
#include "decode_kernels.h"

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
	uint32_t local;
	const DecodeSampleRecord rec = decode_table_item<DecodeSampleRecord>(set, tile0 + blockIdx.x, local);
	(void)decode_sample_tile<kType, kLayout>(rec, local, batch, tile);
}

unsigned long long astc_decode_sample_tiles(uint32_t out_x, uint32_t out_y) { return decode_sample_tiles(out_x, out_y); }

size_t astc_decode_sample_bytes(uint32_t count) { return decode_sample_bytes(count); }

uint32_t astc_decode_sample_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeSampler& sampler,
                                  const DecodeSampleLaunch* grids, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_sample_build(out, of.images.data(), of.streams.data(), format, sampler, grids, count);
}

int astc_decode_sample_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	static const DecodeTableKernel builds[3][2] = DECODE_TENSOR_BUILDS(astc_decode_sample);
	return decode_table_launch(builds, type, layout, d_table, tiles, stream);
}

} // namespace astcd
