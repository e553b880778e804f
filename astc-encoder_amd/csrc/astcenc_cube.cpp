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
	DecodeTensorFormat fmt;
	DecodeLodSampler smp;
	std::vector<DecompressDeviceJob> jobs;
	astcenc_error status = check_lod_call(fn, ctx, entries, entry_count, format, sampler, false, fmt, smp, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeLodLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_cube_grid& g = grids[i];
		SampleGridShape points = { g.out_x, g.out_y, g.dirs, g.dir_row_pitch };
		points.per_point = 3; points.name = "dirs"; points.pitch_name = "dir_row_pitch";
		launches[i].z = g.cube;
		status = check_lod_grid(fn, i, grid_count, entries, entry_count, format, g, points, g.out, "out",
			[&](const astcenc_amd_image_set_entry& en, unsigned int entry, unsigned int l)
			{
				if (en.dim_x != en.dim_y || en.dim_z % 6 != 0)
				{
					backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u x %u: a level of cubes has square faces and six layers a cube", fn, i, grid_count, entry, l,
					            en.dim_x, en.dim_y, en.dim_z);
					return ASTCENC_ERR_BAD_PARAM;
				}
				if ((unsigned long long)g.cube * 6u + 5u >= en.dim_z)
				{
					backend_log("%s: grid %u of %u: cube %u is not inside the %u layers of entry %u (level %u)", fn, i, grid_count, g.cube, en.dim_z, entry, l);
					return ASTCENC_ERR_BAD_PARAM;
				}
				// (a face coordinate is at most s: the tap indices fit 32 bits with room to spare)
				if (en.dim_x > 65536)
				{
					backend_log("%s: grid %u of %u: entry %u (level %u) has faces of %u texels: a level is at most 65536 along x and y", fn, i, grid_count, entry, l, en.dim_x);
					return ASTCENC_ERR_BAD_PARAM;
				}
				return ASTCENC_SUCCESS;
			}, launches[i], tiles);
		if (status != ASTCENC_SUCCESS) return status;
	}

	DecompressLodJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_cube);
}

} // extern "C"
