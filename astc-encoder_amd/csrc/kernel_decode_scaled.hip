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
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <vector>

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
	typedef const __attribute__((address_space(4))) uint8_t* constant_bytes;
	const constant_bytes t = (constant_bytes)reinterpret_cast<uintptr_t>(set);
	const uint32_t count = reinterpret_cast<const __attribute__((address_space(4))) ImageSetTable*>(t)->count;
	const __attribute__((address_space(4))) uint32_t* first = reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(t + image_set_first_offset());
	const uint32_t r = tile0 + blockIdx.x;
	const uint32_t g = image_set_find(first, count, r);
	const DecodeScaledRecord rec = image_set_record<DecodeScaledRecord>(reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(
		t + image_set_records_offset(count) + (size_t)g * sizeof(DecodeScaledRecord)));
	(void)decode_scaled_tile<kType, kLayout>(rec, r - first[g], batch, tile);
}

unsigned long long astc_decode_scaled_tiles(const DecodeScaledLaunch& r, uint32_t data_type, uint32_t block_x, uint32_t block_y)
{
	return decode_scaled_tiles(r.size_x, r.out_x, r.out_y, data_type, block_x, block_y);
}

size_t astc_decode_scaled_bytes(uint32_t count) { return decode_scaled_bytes(count); }

uint32_t astc_decode_scaled_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format, uint32_t filter,
                                  const DecodeScaledLaunch* regions, uint32_t count)
{
	std::vector<DecodeImage> images(entry_count);
	std::vector<const uint8_t*> streams(entry_count);
	for (uint32_t e = 0; e < entry_count; e++)
	{
		const DecodeLaunch& d = entries[e];
		DecodeImage& img = images[e];
		img.data = nullptr;
		img.tabs = static_cast<const DecodeTables*>(d.d_tables);
		img.dim_x = d.dim_x; img.dim_y = d.dim_y; img.dim_z = d.dim_z;
		img.data_type = d.data_type;
		for (int i = 0; i < 4; i++) img.swz[i] = d.swz[i];
		img.block_x = d.block_x; img.block_y = d.block_y; img.block_z = d.block_z;
		img.blocks_x = (d.dim_x + d.block_x - 1) / d.block_x;
		img.blocks_y = (d.dim_y + d.block_y - 1) / d.block_y;
		img.blocks_z = (d.dim_z + d.block_z - 1) / d.block_z;
		img.profile = d.profile;
		decode_image_prepare(img);
		streams[e] = d.d_blocks;
	}
	return decode_scaled_build(out, images.data(), streams.data(), format, filter, regions, count);
}

int astc_decode_scaled_launch(const void* d_table, uint32_t tiles, uint32_t type, uint32_t layout, void* stream)
{
	typedef void (*Kernel)(const ImageSetTable*, uint32_t);
	static const Kernel kernels[3][2] = { { astc_decode_scaled<0, 0>, astc_decode_scaled<0, 1> }, { astc_decode_scaled<1, 0>, astc_decode_scaled<1, 1> },
	                                      { astc_decode_scaled<2, 0>, astc_decode_scaled<2, 1> } };
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
