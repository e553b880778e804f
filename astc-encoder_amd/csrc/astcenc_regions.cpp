// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_decompress_regions_device (include/astcenc_amd.h): windows of device-resident compressed images, many per launch.
// Every entry and every region is checked here, all of them before anything is launched; the backend then decodes the covered
// blocks of all regions as one range of work items (backend_decompress_regions).
// Product library only, like astcenc_set.cpp: the sequential build of oracle/emu has no backend_decompress_regions.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cstring>
#include <vector>

using namespace astcd;

static astcenc_error rc_to_error(int rc)
{
	return rc == 0 ? ASTCENC_SUCCESS : rc == 1 ? ASTCENC_ERR_OUT_OF_MEM : rc == 3 ? ASTCENC_ERR_BAD_PARAM : ASTCENC_ERR_BAD_CONTEXT;
}

extern "C" {

astcenc_error astcenc_amd_decompress_regions_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                    const astcenc_amd_decode_region* regions, unsigned int region_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_decompress_regions_device";
	if (region_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !regions || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;

	std::vector<DecompressDeviceJob> jobs(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		// (`image` is not used: the check's non-null test of it sees the stream's pointer)
		astcenc_error status = (int)en.data_type < ASTCENC_TYPE_U8 || (int)en.data_type > ASTCENC_TYPE_F32 ? ASTCENC_ERR_BAD_PARAM :
		                       check_decompress_device_args(ctx, en.blocks, en.blocks_len, en.blocks, en.dim_x, en.dim_y, en.dim_z, &en.swizzle);
		if (status != ASTCENC_SUCCESS)
		{
			backend_log("%s: entry %u of %u: %s", fn, e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		DecompressDeviceJob& job = jobs[e];
		memset(&job, 0, sizeof(job));
		job.device_blocks = static_cast<const uint8_t*>(en.blocks);
		job.dim_x = en.dim_x; job.dim_y = en.dim_y; job.dim_z = en.dim_z;
		job.data_type = (uint32_t)en.data_type;
		job.swz[0] = en.swizzle.r; job.swz[1] = en.swizzle.g; job.swz[2] = en.swizzle.b; job.swz[3] = en.swizzle.a;
	}

	std::vector<DecodeRegionLaunch> launches(region_count);
	unsigned long long runs = 0;
	for (unsigned int i = 0; i < region_count; i++)
	{
		const astcenc_amd_decode_region& r = regions[i];
		if (r.entry >= entry_count)
		{
			backend_log("%s: region %u of %u: entry %u, the call has %u entries", fn, i, region_count, r.entry, entry_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
		const astcenc_amd_image_set_entry& en = entries[r.entry];
		if (r.size_x == 0 || r.size_y == 0 || r.size_z == 0)
		{
			backend_log("%s: region %u of %u: size %u x %u x %u: a size is zero", fn, i, region_count, r.size_x, r.size_y, r.size_z);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// (64 bits: x + size_x may wrap 32)
		if ((unsigned long long)r.x + r.size_x > en.dim_x || (unsigned long long)r.y + r.size_y > en.dim_y || (unsigned long long)r.z + r.size_z > en.dim_z)
		{
			backend_log("%s: region %u of %u: window %u x %u x %u at (%u, %u, %u) is not inside the %u x %u x %u image of entry %u", fn, i, region_count,
			            r.size_x, r.size_y, r.size_z, r.x, r.y, r.z, en.dim_x, en.dim_y, en.dim_z, r.entry);
			return ASTCENC_ERR_BAD_PARAM;
		}
		const size_t texel = texel_bytes((uint32_t)en.data_type);
		bool overflow = false;
		const size_t tight_row = mul_safe(r.size_x, texel, overflow);
		const size_t row_pitch = r.row_pitch ? r.row_pitch : tight_row;
		const size_t tight_slice = mul_safe(row_pitch, r.size_y, overflow);
		const size_t slice_pitch = r.slice_pitch ? r.slice_pitch : tight_slice;
		(void)mul_safe(slice_pitch, r.size_z, overflow);
		if (overflow || row_pitch < tight_row || slice_pitch < tight_slice)
		{
			backend_log("%s: region %u of %u: row_pitch %zu, slice_pitch %zu: the window needs at least %zu and %zu", fn, i, region_count, r.row_pitch,
			            r.slice_pitch, tight_row, tight_slice);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (row_pitch % texel != 0 || slice_pitch % texel != 0)
		{
			backend_log("%s: region %u of %u: row_pitch %zu, slice_pitch %zu: not multiples of the texel size %zu", fn, i, region_count, r.row_pitch,
			            r.slice_pitch, texel);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// (a null buffer: what the other device calls return for one)
		if (!r.out)
		{
			backend_log("%s: region %u of %u: out is null", fn, i, region_count);
			return ASTCENC_ERR_BAD_CONTEXT;
		}
		if (reinterpret_cast<uintptr_t>(r.out) % texel != 0)
		{
			backend_log("%s: region %u of %u: out %p is not aligned to the texel size %zu", fn, i, region_count, r.out, texel);
			return ASTCENC_ERR_BAD_PARAM;
		}
		DecodeRegionLaunch& l = launches[i];
		l.entry = r.entry;
		l.x = r.x; l.y = r.y; l.z = r.z;
		l.size_x = r.size_x; l.size_y = r.size_y; l.size_z = r.size_z;
		l.d_out = r.out;
		l.row_pitch = row_pitch; l.slice_pitch = slice_pitch;
		runs += astc_decode_region_runs(l, ctx->config.block_x, ctx->config.block_y, ctx->config.block_z);
		if (runs > 0xFFFFFFFFull)
		{
			backend_log("%s: region %u of %u: more than 2^32 - 1 runs of blocks in all", fn, i, region_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}

	DecompressRegionsJob job;
	memset(&job, 0, sizeof(job));
	job.entries = jobs.data();
	job.entry_count = entry_count;
	job.regions = launches.data();
	job.region_count = region_count;
	job.stream = hip_stream;
	const astcenc_error status = rc_to_error(backend_decompress_regions(ctx->backend, job));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: a buffer or hip_stream is not on the device of entry 0's blocks", fn);
	return status;
}

} // extern "C"
