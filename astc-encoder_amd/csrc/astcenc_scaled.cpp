// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_decompress_scaled_tensors_device (include/astcenc_amd.h): windows of device-resident compressed images resampled
// to a size of their own and written as tensors -- the random resized crop of a training loader -- many per launch.  The format,
// the filter, every entry and every region are checked here, all of them before anything is launched; the backend then covers
// the output tiles of all regions as one range of work items (backend_decompress_scaled).
// Product library only, like astcenc_tensors.cpp.
#include "regions_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_decompress_scaled_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                           const astcenc_amd_tensor_format* format, astcenc_amd_window_filter filter,
                                                           const astcenc_amd_scaled_region* regions, unsigned int region_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_decompress_scaled_tensors_device";
	if (region_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !regions || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	astcenc_error status = check_tensor_format(fn, format);
	if (status != ASTCENC_SUCCESS) return status;
	if ((int)filter != ASTCENC_AMD_WINDOW_BILINEAR && (int)filter != ASTCENC_AMD_WINDOW_BOX)
	{
		backend_log("%s: filter %d: not a window filter", fn, (int)filter);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (ctx->config.block_z > 1)
	{
		backend_log("%s: the context's footprint %ux%ux%u is 3D: windows of 2D footprints are resampled", fn, ctx->config.block_x, ctx->config.block_y,
		            ctx->config.block_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	DecodeTensorFormat fmt;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecompressDeviceJob> jobs;
	status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeScaledLaunch> launches(region_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < region_count; i++)
	{
		const astcenc_amd_scaled_region& r = regions[i];
		// (entry, zero window sizes, the window and its slice inside the image)
		status = check_window(fn, i, region_count, entries, entry_count, r.entry, r.x, r.y, r.z, r.size_x, r.size_y, 1);
		if (status != ASTCENC_SUCCESS) return status;
		if (r.out_x == 0 || r.out_y == 0 || r.size_x > 65535 || r.size_y > 65535 || r.out_x > 65535 || r.out_y > 65535)
		{
			backend_log("%s: region %u of %u: window %u x %u to %u x %u: every size is 1 to 65535", fn, i, region_count, r.size_x, r.size_y, r.out_x, r.out_y);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (r.flags & ~(ASTCENC_AMD_TENSOR_FLIP_X | ASTCENC_AMD_TENSOR_FLIP_Y))
		{
			backend_log("%s: region %u of %u: flags 0x%x: unknown bits", fn, i, region_count, r.flags);
			return ASTCENC_ERR_BAD_PARAM;
		}
		TensorPitches pitches = { r.row_pitch, 0, r.plane_pitch };
		status = check_output_tensor(fn, "region", i, region_count, format, r.out_x, r.out_y, 0, pitches, r.out);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeScaledLaunch& l = launches[i];
		l.entry = r.entry;
		l.x = r.x; l.y = r.y; l.z = r.z;
		l.size_x = r.size_x; l.size_y = r.size_y;
		l.out_x = r.out_x; l.out_y = r.out_y;
		l.flags = r.flags;
		l.d_out = r.out;
		l.row_pitch = pitches.row; l.plane_pitch = pitches.plane;
		tiles += astc_decode_scaled_tiles(l, (uint32_t)entries[r.entry].data_type, ctx->config.block_x, ctx->config.block_y);
		if (tiles > 0xFFFFFFFFull)
		{
			backend_log("%s: region %u of %u: more than 2^32 - 1 output tiles in all", fn, i, region_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}

	DecompressScaledJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.filter = (uint32_t)filter;
	job.regions = launches.data();
	job.region_count = region_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_scaled);
}

} // extern "C"
