// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_cube_tensors_device (include/astcenc_amd.h): device-resident compressed cube maps -- one level or a mip
// chain -- sampled at buffers of directions with a level of detail per point: the reflection vectors of a probe lookup, the view
// rays of a sky box, the normals of an environment-lighting pass -- and written as tensors, many grids per launch.  The format,
// the sampler, every entry and every grid are checked here, all of them before anything is launched; the backend then covers the
// tiles of all grids as one range of work items (backend_decompress_cube).  The directions and the levels of
// detail themselves are data: none of them is an error.
// Product library only, like astcenc_lod.cpp.
#include "sample_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_cube_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                     const astcenc_amd_tensor_format* format, const astcenc_amd_cube_sampler* sampler,
                                                     const astcenc_amd_cube_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_cube_tensors_device";
	if (grid_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !grids || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	astcenc_error status = check_tensor_format(fn, format);
	if (status != ASTCENC_SUCCESS) return status;
	if (!sampler)
	{
		backend_log("%s: sampler is null", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (a cube has no address modes: its edges are its neighbours')
	status = check_sample_modes(fn, (int)sampler->filter, ASTCENC_AMD_ADDRESS_CLAMP, ASTCENC_AMD_ADDRESS_CLAMP);
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

	std::vector<DecodeCubeLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_cube_grid& g = grids[i];
		status = check_lod_chain(fn, i, grid_count, g.first_entry, g.level_count, entry_count);
		if (status != ASTCENC_SUCCESS) return status;
		for (unsigned int l = 0; l < g.level_count; l++)
		{
			const astcenc_amd_image_set_entry& en = entries[g.first_entry + l];
			if (en.dim_x != en.dim_y || en.dim_z % 6 != 0)
			{
				backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u x %u: a level of cubes has square faces and six layers a cube", fn, i, grid_count,
				            g.first_entry + l, l, en.dim_x, en.dim_y, en.dim_z);
				return ASTCENC_ERR_BAD_PARAM;
			}
			if ((unsigned long long)g.cube * 6u + 5u >= en.dim_z)
			{
				backend_log("%s: grid %u of %u: cube %u is not inside the %u layers of entry %u (level %u)", fn, i, grid_count, g.cube, en.dim_z, g.first_entry + l, l);
				return ASTCENC_ERR_BAD_PARAM;
			}
			// (a face coordinate is at most s: the tap indices fit 32 bits with room to spare)
			if (en.dim_x > 65536)
			{
				backend_log("%s: grid %u of %u: entry %u (level %u) has faces of %u texels: a level is at most 65536 along x and y", fn, i, grid_count, g.first_entry + l, l,
				            en.dim_x);
				return ASTCENC_ERR_BAD_PARAM;
			}
		}
		status = check_lod_pitch(fn, i, grid_count, g.lod_bias, g.lod_row_pitch, g.out_x);
		if (status != ASTCENC_SUCCESS) return status;
		CubeGridShape shape = { g.out_x, g.out_y, g.dirs, g.dir_row_pitch, g.out, g.row_pitch, g.plane_pitch };
		status = check_cube_grid(fn, i, grid_count, format, shape);
		if (status != ASTCENC_SUCCESS) return status;
		size_t lod_row_pitch = g.lod_row_pitch;
		status = check_lod_buffer(fn, i, grid_count, g.lod, lod_row_pitch, g.out_x, g.out_y);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeCubeLaunch& l = launches[i];
		l.first_entry = g.first_entry; l.level_count = g.level_count;
		l.cube = g.cube;
		l.out_x = g.out_x; l.out_y = g.out_y;
		l.d_dirs = g.dirs;
		l.dir_row_pitch = shape.dir_row_pitch;
		l.d_lod = g.lod;
		l.lod_row_pitch = lod_row_pitch;
		l.lod_bias = g.lod_bias;
		l.d_out = g.out;
		l.row_pitch = shape.row_pitch; l.plane_pitch = shape.plane_pitch;
		if (!add_sample_tiles(fn, i, grid_count, g.out_x, g.out_y, tiles)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecodeCubeSampler smp;
	smp.filter = (uint32_t)sampler->filter;
	smp.mip_filter = (uint32_t)sampler->mip_filter;
	DecompressCubeJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_cube);
}

} // extern "C"
