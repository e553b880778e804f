// SPDX-License-Identifier: Apache-2.0
// Decompression kernel: one wavefront per run of DECODE_BATCH consecutive blocks of a block row, texels written
// straight into the output image in HBM (astcenc_decompress_image; ref: Source/astcenc_entry.cpp:1274-1390).
#define ASTC_VARIANT v_dec
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_decode.h"
#include "decode_regions.h"
#include "decode_tensors.h"
#include "decode_kernels.h"

namespace astcd {

/* One block is a few hundred instructions that keep under half of a wavefront busy, so every wavefront takes a run of
 * DECODE_BATCH consecutive blocks of one block row and decodes it together (decode_row_batch).  The grid is (runs per block
 * row, block rows, layers of blocks): a run's place in the image needs no division.  `row0` / `layer0`: the launch covers
 * block rows [row0, row0 + gridDim.y) and layers [layer0, layer0 + gridDim.z) of the stream (astc_decode_launch). */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8)))      // (LDS allows 5.75 waves per SIMD: keep the registers under that)
astc_decompress_blocks(const uint8_t* __restrict__ blocks, DecodeImage img, uint32_t row0, uint32_t layer0)
{
	__shared__ DecodeBatch batch;
	const uint32_t bx0 = blockIdx.x * (uint32_t)DECODE_BATCH;
	const uint32_t left = img.blocks_x - bx0;
	decode_row_batch(img, blocks, bx0, row0 + blockIdx.y, layer0 + blockIdx.z, (int)(left < (uint32_t)DECODE_BATCH ? left : (uint32_t)DECODE_BATCH), batch);
}

/* An image set (astcenc_amd_compress_images_device's counterpart): the runs of every entry back to back on a 1D grid, the
 * entry of a run found in the table (image_set.h), its place in the entry -- run, block row, layer -- split off with scalar
 * arithmetic.  `run0`: the launch covers runs [run0, run0 + gridDim.x) of the set (astc_decode_set_launch). */
struct DecodeSetEntry {
	DecodeImage img;
	const uint8_t* blocks;
	uint32_t runs_x;          // runs per block row: ceil(blocks_x / DECODE_BATCH)
	uint32_t runs_xy;         // ... per layer of blocks
};

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8)))
astc_decompress_set(const ImageSetTable* __restrict__ set, uint32_t run0)
{
	__shared__ DecodeBatch batch;
	uint32_t local;
	const DecodeSetEntry rec = decode_table_item<DecodeSetEntry>(set, run0 + blockIdx.x, local);
	const uint32_t bz = local / rec.runs_xy;
	const uint32_t in_layer = local - bz * rec.runs_xy;
	const uint32_t by = in_layer / rec.runs_x;
	const uint32_t bx0 = (in_layer - by * rec.runs_x) * (uint32_t)DECODE_BATCH;
	const uint32_t left = rec.img.blocks_x - bx0;
	decode_row_batch(rec.img, rec.blocks, bx0, by, bz, (int)(left < (uint32_t)DECODE_BATCH ? left : (uint32_t)DECODE_BATCH), batch);
}

/* Windows of compressed images (astcenc_amd_decompress_regions_device): the runs of every region back to back on a 1D grid, a
 * run's region found in the table, its window decoded into the region's own buffer (decode_regions.h).  `run0`: the launch
 * covers runs [run0, run0 + gridDim.x) of the call (astc_decode_regions_launch). */
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8)))
astc_decode_regions(const ImageSetTable* __restrict__ set, uint32_t run0)
{
	__shared__ DecodeBatch batch;
	uint32_t local;
	const DecodeRegionRecord rec = decode_table_item<DecodeRegionRecord>(set, run0 + blockIdx.x, local);
	DecodeStore store;
	decode_region_run(rec, local, batch, store);
}

/* Windows decoded into tensors (astcenc_amd_decompress_tensors_device): astc_decode_regions with the tensor policies of
 * decode_tensors.h -- the same table shape, lookup and grid; the record also carries the call's format, and the texels leave
 * converted, scaled and placed (TensorStore, TensorWindow).  One build per tensor type and layout, which hold for a call. */
template <uint32_t kType, uint32_t kLayout>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 8)))
astc_decode_tensors(const ImageSetTable* __restrict__ set, uint32_t run0)
{
	__shared__ DecodeBatch batch;
	uint32_t local;
	const DecodeTensorRecord rec = decode_table_item<DecodeTensorRecord>(set, run0 + blockIdx.x, local);
	decode_tensor_run<kType, kLayout>(rec, local, batch);
}

size_t astc_decode_tables_bytes() { return sizeof(DecodeTables); }

void astc_decode_tables_build(void* out, uint32_t block_x, uint32_t block_y, uint32_t block_z)
{
	decode_tables_build(*static_cast<DecodeTables*>(out), (int)block_x, (int)block_y, (int)block_z);
}

int astc_decode_launch(const DecodeLaunch& d)
{
	const DecodeImage img = decode_image_of(d, d.d_image);
	// Grid y / z hold block rows / layers of blocks, at most 65535 each: a taller stream (more than 262 140 texel rows at the
	// smallest footprint, or as many slices) is covered by several launches, each told where its rows and layers start.  The
	// image record stays the whole image's, so every address is formed from the real dimensions.
	static const uint32_t limit = decode_grid_limit(65535u);
	const uint32_t runs = (img.blocks_x + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH;
	for (uint32_t layer0 = 0; layer0 < img.blocks_z; layer0 += limit)
	{
		const uint32_t layers = img.blocks_z - layer0 < limit ? img.blocks_z - layer0 : limit;
		for (uint32_t row0 = 0; row0 < img.blocks_y; row0 += limit)
		{
			const uint32_t rows = img.blocks_y - row0 < limit ? img.blocks_y - row0 : limit;
			hipLaunchKernelGGL(astc_decompress_blocks, dim3(runs, rows, layers), dim3(64), 0, static_cast<hipStream_t>(d.stream), d.d_blocks, img, row0, layer0);
		}
	}
	return (int)hipGetLastError();
}

size_t astc_decode_set_bytes(uint32_t count) { return decode_table_bytes<DecodeSetEntry>(count); }

uint32_t astc_decode_set_build(void* out, const DecodeLaunch* entries, uint32_t count)
{
	uint32_t* first;
	DecodeSetEntry* rec = decode_table_begin<DecodeSetEntry>(out, astc_decode_set_bytes(count), count, first);
	uint32_t runs = 0;
	for (uint32_t e = 0; e < count; e++)
	{
		rec[e].img = decode_image_of(entries[e], entries[e].d_image);
		rec[e].blocks = entries[e].d_blocks;
		rec[e].runs_x = (rec[e].img.blocks_x + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH;
		rec[e].runs_xy = rec[e].runs_x * rec[e].img.blocks_y;
		first[e] = runs;
		runs += rec[e].runs_xy * rec[e].img.blocks_z;
	}
	return decode_table_finish(out, count, runs);
}

int astc_decode_set_launch(const void* d_table, uint32_t runs, void* stream) { return decode_table_launch(astc_decompress_set, d_table, runs, stream); }

unsigned long long astc_decode_region_runs(const DecodeRegionLaunch& r, uint32_t block_x, uint32_t block_y, uint32_t block_z)
{
	return decode_region_runs(r.x, r.y, r.z, r.size_x, r.size_y, r.size_z, block_x, block_y, block_z);
}

size_t astc_decode_regions_bytes(uint32_t count) { return decode_regions_bytes(count); }

uint32_t astc_decode_regions_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeRegionLaunch* regions, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_regions_build(out, of.images.data(), of.streams.data(), regions, count);
}

int astc_decode_regions_launch(const void* d_table, uint32_t runs, void* stream) { return decode_table_launch(astc_decode_regions, d_table, runs, stream); }

size_t astc_decode_tensors_bytes(uint32_t count) { return decode_tensors_bytes(count); }

uint32_t astc_decode_tensors_build(void* out, const DecodeLaunch* entries, uint32_t entry_count, const DecodeTensorFormat& format,
                                   const DecodeTensorLaunch* regions, uint32_t count)
{
	const DecodeEntries of(entries, entry_count);
	return decode_tensors_build(out, of.images.data(), of.streams.data(), format, regions, count);
}

int astc_decode_tensors_launch(const void* d_table, uint32_t runs, uint32_t type, uint32_t layout, void* stream)
{
	static const DecodeTableKernel builds[3][2] = DECODE_TENSOR_BUILDS(astc_decode_tensors);
	return decode_table_launch(builds, type, layout, d_table, runs, stream);
}

} // namespace astcd
