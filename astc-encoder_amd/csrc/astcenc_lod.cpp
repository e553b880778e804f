// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_lod_tensors_device (include/astcenc_amd.h): device-resident compressed mip chains sampled at buffers of
// normalised coordinates with a level of detail per point -- the UV and LOD buffers of a rasteriser, a neural-texture trainer, a
// texture-space shading pass -- and written as tensors, many grids per launch.  The format, the sampler, every entry and every
// grid are checked here, all of them before anything is launched; the backend then covers the tiles of all grids as one range of
// work items (backend_decompress_lod).  The coordinates and the levels of detail themselves are data: none of
// them is an error.
// Product library only, like astcenc_sample.cpp.
#include "sample_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_lod_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                    const astcenc_amd_tensor_format* format, const astcenc_amd_lod_sampler* sampler,
                                                    const astcenc_amd_lod_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_lod_tensors_device";
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
	status = check_mip_level_filter(fn, (int)sampler->mip_filter);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_sample_footprint(fn, ctx);
	if (status != ASTCENC_SUCCESS) return status;
	DecodeTensorFormat fmt;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecompressDeviceJob> jobs;
	status = check_sample_entries(fn, ctx, entries, entry_count, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeLodLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_lod_grid& g = grids[i];
		status = check_lod_chain(fn, i, grid_count, g.first_entry, g.level_count, entry_count);
		if (status != ASTCENC_SUCCESS) return status;
		for (unsigned int l = 0; l < g.level_count; l++)
		{
			const astcenc_amd_image_set_entry& en = entries[g.first_entry + l];
			if (g.z >= en.dim_z)
			{
				backend_log("%s: grid %u of %u: slice %u is not inside the %u x %u x %u image of entry %u (level %u)", fn, i, grid_count, g.z, en.dim_x, en.dim_y,
				            en.dim_z, g.first_entry + l, l);
				return ASTCENC_ERR_BAD_PARAM;
			}
			// (a level coordinate is u W: within 2^30 for |u| <= 2^14)
			if (en.dim_x > 65536 || en.dim_y > 65536)
			{
				backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u texels: a level is at most 65536 along x and y", fn, i, grid_count, g.first_entry + l, l,
				            en.dim_x, en.dim_y);
				return ASTCENC_ERR_BAD_PARAM;
			}
		}
		status = check_lod_pitch(fn, i, grid_count, g.lod_bias, g.lod_row_pitch, g.out_x);
		if (status != ASTCENC_SUCCESS) return status;
		SampleGridShape shape = { g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch };
		status = check_sample_grid(fn, i, grid_count, format, shape);
		if (status != ASTCENC_SUCCESS) return status;
		size_t lod_row_pitch = g.lod_row_pitch;
		status = check_lod_buffer(fn, i, grid_count, g.lod, lod_row_pitch, g.out_x, g.out_y);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeLodLaunch& l = launches[i];
		l.first_entry = g.first_entry; l.level_count = g.level_count;
		l.z = g.z;
		l.out_x = g.out_x; l.out_y = g.out_y;
		l.d_coords = g.coords;
		l.coord_row_pitch = shape.coord_row_pitch;
		l.d_lod = g.lod;
		l.lod_row_pitch = lod_row_pitch;
		l.lod_bias = g.lod_bias;
		l.d_out = g.out;
		l.row_pitch = shape.row_pitch; l.plane_pitch = shape.plane_pitch;
		if (!add_sample_tiles(fn, i, grid_count, g.out_x, g.out_y, tiles)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecodeLodSampler smp;
	smp.filter = (uint32_t)sampler->filter; smp.address_x = (uint32_t)sampler->address_x; smp.address_y = (uint32_t)sampler->address_y;
	smp.mip_filter = (uint32_t)sampler->mip_filter;
	DecompressLodJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_lod);
}

} // extern "C"
