// SPDX-License-Identifier: Apache-2.0
// Compressed cube maps sampled by direction at a level of detail per point (astcenc_amd_sample_cube_tensors_device): one
// wavefront per tile of 64 points of a grid, the lane is the point; the lane finds its face and face coordinates, the wave walks
// the distinct mip levels its points need and runs the coordinate sampler's pipeline once per level over blocks of whichever
// faces the taps reach, then every lane blends its one or two levels in registers (decode_cube.h on decode_lod.h's level walk).
// A translation unit of its own, so that kernel_decode_lod.hip and its kernels are what they were.
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_cube.h"
#include "decode_kernels.h"

namespace astcd {

// LDS of a workgroup: what astc_lod_sample has -- DecodeBatch and the batch's block list, nothing else.
static_assert(sizeof(DecodeBatch) + sizeof(SampleTile) == 7168, "astc_cube_sample: DecodeBatch (7040 B) and the list of a batch's blocks (128 B)");

/* The level records of a grid in the table: level l (uniform) read word by word with scalar loads. */
struct CubeLevelsOfGrid {
	constant_bytes at;
	__device__ DecodeLodLevel operator()(uint32_t l) const
	{
		return image_set_record<DecodeLodLevel>(reinterpret_cast<constant_words>(at + (size_t)l * sizeof(DecodeLodLevel)));
	}
};

/* The tiles of every grid back to back on a 1D grid, a tile's grid found in the table (image_set.h).  `tile0`: the launch covers
 * tiles [tile0, tile0 + gridDim.x) of the call.  One build per tensor type and layout, which hold for a call; the filters and
 * every level's data type are wave-uniform values of the records. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64)
astc_cube_sample(const ImageSetTable* __restrict__ set, uint32_t tile0)
{
	__shared__ DecodeBatch batch;
	__shared__ SampleTile tile;
	uint32_t local;
	const DecodeCubeRecord rec = decode_table_item<DecodeCubeRecord>(set, tile0 + blockIdx.x, local);
	const CubeLevelsOfGrid levels = { (constant_bytes)reinterpret_cast<uintptr_t>(set) + rec.levels };
	(void)decode_cube_tile<kType, kLayout>(rec, levels, local, batch, tile);
}

size_t astc_decode_cube_bytes(const DecodeLodLaunch* grids, uint32_t count) { return decode_cube_bytes(grids, count); }

uint32_t astc_decode_cube_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                const DecodeLodLaunch* grids, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_cube_build(out, of.images.data(), of.streams.data(), format, sampler, grids, count);
}

int astc_decode_cube_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	static const DecodeTableKernel builds[3][2] = DECODE_TENSOR_BUILDS(astc_cube_sample);
	return decode_table_launch(builds, type, layout, d_table, tiles, stream);
}

} // namespace astcd
