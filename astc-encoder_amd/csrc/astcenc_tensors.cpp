// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_decompress_tensors_device (include/astcenc_amd.h): windows of device-resident compressed images decoded straight
// into tensors -- converted, scaled, mirrored, planar or interleaved -- many per launch.  The format, every entry and every region
// are checked here, all of them before anything is launched; the backend then decodes the covered blocks of all regions as one
// range of work items (backend_decompress_tensors).
// Product library only, like astcenc_regions.cpp.
#include "regions_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_decompress_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                    const astcenc_amd_tensor_format* format,
                                                    const astcenc_amd_tensor_region* regions, unsigned int region_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_decompress_tensors_device";
	if (region_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !regions || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	astcenc_error status = check_tensor_format(fn, format);
	if (status != ASTCENC_SUCCESS) return status;
	DecodeTensorFormat fmt;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecompressDeviceJob> jobs;
	status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeTensorLaunch> launches(region_count);
	unsigned long long runs = 0;
	for (unsigned int i = 0; i < region_count; i++)
	{
		const astcenc_amd_tensor_region& r = regions[i];
		status = check_window(fn, i, region_count, entries, entry_count, r.entry, r.x, r.y, r.z, r.size_x, r.size_y, r.size_z);
		if (status != ASTCENC_SUCCESS) return status;
		if (r.flags & ~(ASTCENC_AMD_TENSOR_FLIP_X | ASTCENC_AMD_TENSOR_FLIP_Y))
		{
			backend_log("%s: region %u of %u: flags 0x%x: unknown bits", fn, i, region_count, r.flags);
			return ASTCENC_ERR_BAD_PARAM;
		}
		TensorPitches pitches = { r.row_pitch, r.slice_pitch, r.plane_pitch };
		status = check_output_tensor(fn, "region", i, region_count, format, r.size_x, r.size_y, r.size_z, pitches, r.out);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeTensorLaunch& l = launches[i];
		l.entry = r.entry;
		l.x = r.x; l.y = r.y; l.z = r.z;
		l.size_x = r.size_x; l.size_y = r.size_y; l.size_z = r.size_z;
		l.flags = r.flags;
		l.d_out = r.out;
		l.row_pitch = pitches.row; l.slice_pitch = pitches.slice; l.plane_pitch = pitches.plane;
		DecodeRegionLaunch window;
		memset(&window, 0, sizeof(window));
		window.x = r.x; window.y = r.y; window.z = r.z;
		window.size_x = r.size_x; window.size_y = r.size_y; window.size_z = r.size_z;
		if (!add_window_runs(fn, i, region_count, ctx, window, runs)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecompressTensorsJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.regions = launches.data();
	job.region_count = region_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_tensors);
}

} // extern "C"
