// SPDX-License-Identifier: Apache-2.0
// The gradients of the volume sampler (astcenc_amd_sample_volume_grad_device): one wavefront per tile of 64 points of a grid,
// the lane is the point; the wave walks the distinct mip levels its points need as astc_volume_sample does, keeps all eight
// taps of a trilinear point and, per level, four binary64 values a lane -- the upstream gradient against the differences along
// x, y and z and against the level's sample -- which the lane blends into d loss / d (u, v, w) and d loss / d lambda
// (decode_volume_grad.h).  A translation unit of its own, so that kernel_decode_volume.hip and its kernels are what they were.
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_volume_grad.h"
#include "decode_kernels.h"

namespace astcd {

// LDS of a workgroup: what astc_volume_sample has -- DecodeBatch and the batch's block list, nothing else.
static_assert(sizeof(DecodeBatch) + sizeof(SampleTile) == 7168, "astc_volume_grad: DecodeBatch (7040 B) and the list of a batch's blocks (128 B)");

/* The level records of a grid in the table: level l (uniform) read word by word with scalar loads. */
struct VolumeGradLevelsOfGrid {
	constant_bytes at;
	__device__ DecodeLodLevel operator()(uint32_t l) const
	{
		return image_set_record<DecodeLodLevel>(reinterpret_cast<constant_words>(at + (size_t)l * sizeof(DecodeLodLevel)));
	}
};

/* The tiles of every grid back to back on a 1D grid, as astc_volume_sample has them.  One build per tensor type and layout of
 * grad_out, which hold for a call. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64)
astc_volume_grad(const ImageSetTable* __restrict__ set, uint32_t tile0)
{
	__shared__ DecodeBatch batch;
	__shared__ SampleTile tile;
	uint32_t local;
	const DecodeVolumeGradRecord rec = decode_table_item<DecodeVolumeGradRecord>(set, tile0 + blockIdx.x, local);
	const VolumeGradLevelsOfGrid levels = { (constant_bytes)reinterpret_cast<uintptr_t>(set) + rec.vol.levels };
	(void)decode_volume_grad_tile<kType, kLayout>(rec, levels, local, batch, tile);
}

size_t astc_decode_volume_grad_bytes(const DecodeLodGradLaunch* grids, uint32_t count) { return decode_volume_grad_bytes(grids, count); }

uint32_t astc_decode_volume_grad_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                       const DecodeLodGradLaunch* grids, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_volume_grad_build(out, of.images.data(), of.streams.data(), format, sampler, grids, count);
}

int astc_decode_volume_grad_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	static const DecodeTableKernel builds[3][2] = DECODE_TENSOR_BUILDS(astc_volume_grad);
	return decode_table_launch(builds, type, layout, d_table, tiles, stream);
}

} // namespace astcd
