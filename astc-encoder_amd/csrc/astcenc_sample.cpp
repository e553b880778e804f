// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_tensors_device (include/astcenc_amd.h): device-resident compressed images sampled at buffers of coordinates
// -- the UV buffer of a rasteriser, a warp field, a rotated crop -- and written as tensors, many grids per launch.  The format,
// the sampler, every entry and every grid are checked here, all of them before anything is launched; the backend then covers the
// tiles of all grids as one range of work items (backend_decompress_sample).  The coordinates themselves are
// data: none of them is an error.
// Product library only, like astcenc_scaled.cpp.
#include "sample_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                const astcenc_amd_tensor_format* format, const astcenc_amd_sampler* sampler,
                                                const astcenc_amd_sample_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_tensors_device";
	if (grid_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !grids || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	astcenc_error status = check_tensor_format(fn, format);
	if (status != ASTCENC_SUCCESS) return status;
	if (!sampler)
	{
		backend_log("%s: sampler is null", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	status = check_sample_modes(fn, (int)sampler->filter, (int)sampler->address_x, (int)sampler->address_y);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_sample_footprint(fn, ctx);
	if (status != ASTCENC_SUCCESS) return status;
	DecodeTensorFormat fmt;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecompressDeviceJob> jobs;
	status = check_sample_entries(fn, ctx, entries, entry_count, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeSampleLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_sample_grid& g = grids[i];
		if (g.entry >= entry_count)
		{
			backend_log("%s: grid %u of %u: entry %u, the call has %u entries", fn, i, grid_count, g.entry, entry_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (g.z >= entries[g.entry].dim_z)
		{
			backend_log("%s: grid %u of %u: slice %u is not inside the %u x %u x %u image of entry %u", fn, i, grid_count, g.z, entries[g.entry].dim_x,
			            entries[g.entry].dim_y, entries[g.entry].dim_z, g.entry);
			return ASTCENC_ERR_BAD_PARAM;
		}
		SampleGridShape shape = { g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch };
		status = check_sample_grid(fn, i, grid_count, format, shape);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeSampleLaunch& l = launches[i];
		l.entry = g.entry;
		l.z = g.z;
		l.out_x = g.out_x; l.out_y = g.out_y;
		l.d_coords = g.coords;
		l.coord_row_pitch = shape.coord_row_pitch;
		l.d_out = g.out;
		l.row_pitch = shape.row_pitch; l.plane_pitch = shape.plane_pitch;
		if (!add_sample_tiles(fn, i, grid_count, g.out_x, g.out_y, tiles)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecodeSampler smp;
	smp.filter = (uint32_t)sampler->filter; smp.address_x = (uint32_t)sampler->address_x; smp.address_y = (uint32_t)sampler->address_y;
	DecompressSampleJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_sample);
}

} // extern "C"
