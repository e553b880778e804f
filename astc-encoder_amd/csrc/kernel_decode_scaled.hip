// SPDX-License-Identifier: Apache-2.0
// Scaled windows decoded into tensors (astcenc_amd_decompress_scaled_tensors_device): one wavefront per tile of a region's
// output -- up to 64 output columns by up to 8 output rows -- which decodes the blocks its taps reach into LDS with the
// decoder's own routine and filters them there (decode_scaled.h).  A translation unit of its own, so that kernel_decode.hip
// and its kernels are what they were.
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_scaled.h"
#include "decode_kernels.h"

namespace astcd {

/* The tiles of every region back to back on a 1D grid, a tile's region found in the table (image_set.h).  `tile0`: the launch
 * covers tiles [tile0, tile0 + gridDim.x) of the call.  One build per tensor type and layout, which hold for a call; the
 * filter and the entry's data type are wave-uniform values of the record.
 * LDS: DecodeBatch (7040 B) + ScaledTile (6144 B staging, 3072 B carried row sums, 1152 B taps) = 17408 B a workgroup, nine
 * workgroups per CU (160 KiB); the band sums -- 8 rows x 4 components of binary64 -- are 64 of the kernel's registers, which
 * allow two waves per SIMD, eight workgroups per CU. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64)
astc_decode_scaled(const ImageSetTable* __restrict__ set, uint32_t tile0)
{
	__shared__ DecodeBatch batch;
	__shared__ ScaledTile tile;
	uint32_t local;
	const DecodeScaledRecord rec = decode_table_item<DecodeScaledRecord>(set, tile0 + blockIdx.x, local);
	(void)decode_scaled_tile<kType, kLayout>(rec, local, batch, tile);
}

unsigned long long astc_decode_scaled_tiles(const DecodeScaledLaunch& r, uint32_t data_type, uint32_t block_x, uint32_t block_y)
{
	return decode_scaled_tiles(r.size_x, r.out_x, r.out_y, data_type, block_x, block_y);
}

size_t astc_decode_scaled_bytes(uint32_t count) { return decode_scaled_bytes(count); }

uint32_t astc_decode_scaled_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, uint32_t filter,
                                  const DecodeScaledLaunch* regions, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_scaled_build(out, of.images.data(), of.streams.data(), format, filter, regions, count);
}

int astc_decode_scaled_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	static const DecodeTableKernel builds[3][2] = DECODE_TENSOR_BUILDS(astc_decode_scaled);
	return decode_table_launch(builds, type, layout, d_table, tiles, stream);
}

} // namespace astcd
