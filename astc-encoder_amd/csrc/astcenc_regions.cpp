// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_decompress_regions_device (include/astcenc_amd.h): windows of device-resident compressed images, many per launch.
// Every entry and every region is checked here, all of them before anything is launched; the backend then decodes the covered
// blocks of all regions as one range of work items (backend_decompress_regions).
// Product library only, like astcenc_set.cpp: the sequential build of oracle/emu has no backend_decompress_regions.
#include "regions_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_decompress_regions_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                    const astcenc_amd_decode_region* regions, unsigned int region_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_decompress_regions_device";
	if (region_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !regions || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;

	std::vector<DecompressDeviceJob> jobs;
	const astcenc_error entries_status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (entries_status != ASTCENC_SUCCESS) return entries_status;

	std::vector<DecodeRegionLaunch> launches(region_count);
	unsigned long long runs = 0;
	for (unsigned int i = 0; i < region_count; i++)
	{
		const astcenc_amd_decode_region& r = regions[i];
		const astcenc_error window_status = check_window(fn, i, region_count, entries, entry_count, r.entry, r.x, r.y, r.z, r.size_x, r.size_y, r.size_z);
		if (window_status != ASTCENC_SUCCESS) return window_status;
		const astcenc_amd_image_set_entry& en = entries[r.entry];
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
		if (!add_window_runs(fn, i, region_count, ctx, l, runs)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecompressRegionsJob job;
	memset(&job, 0, sizeof(job));
	job.regions = launches.data();
	job.region_count = region_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_regions);
}

} // extern "C"
