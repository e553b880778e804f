// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_volume_tensors_device (include/astcenc_amd.h): device-resident compressed volumes -- one level or a mip
// chain, of 2D footprints over slices or of 3D footprints -- sampled at buffers of normalised (u, v, w) triples with a level of
// detail per point: the samples of a ray marcher through a CT or simulation volume, a fog or density grid, a 3D colour LUT, the
// feature grid of a neural field -- and written as tensors, many grids per launch.  The format, the sampler, every entry and
// every grid are checked here, all of them before anything is launched; the backend then covers the tiles of all grids as one
// range of work items (backend_decompress_volume).  The coordinates and the levels of detail themselves are
// data: none of them is an error.
// Product library only, like astcenc_lod.cpp.
#include "sample_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_volume_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                       const astcenc_amd_tensor_format* format, const astcenc_amd_volume_sampler* sampler,
                                                       const astcenc_amd_volume_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_volume_tensors_device";
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
	status = check_volume_address_z(fn, (int)sampler->address_z);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_mip_level_filter(fn, (int)sampler->mip_filter);
	if (status != ASTCENC_SUCCESS) return status;
	// (every footprint is sampled here: no check_sample_footprint)
	DecodeTensorFormat fmt;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecompressDeviceJob> jobs;
	status = check_volume_entries(fn, ctx, entries, entry_count, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	std::vector<DecodeVolumeLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_volume_grid& g = grids[i];
		status = check_lod_chain(fn, i, grid_count, g.first_entry, g.level_count, entry_count);
		if (status != ASTCENC_SUCCESS) return status;
		for (unsigned int l = 0; l < g.level_count; l++)
		{
			const astcenc_amd_image_set_entry& en = entries[g.first_entry + l];
			// (a level coordinate is u W: within 2^30 for |u| <= 2^14)
			if (en.dim_x > 65536 || en.dim_y > 65536 || en.dim_z > 65536)
			{
				backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u x %u texels: a level is at most 65536 along x, y and z", fn, i, grid_count, g.first_entry + l,
				            l, en.dim_x, en.dim_y, en.dim_z);
				return ASTCENC_ERR_BAD_PARAM;
			}
		}
		status = check_lod_pitch(fn, i, grid_count, g.lod_bias, g.lod_row_pitch, g.out_x);
		if (status != ASTCENC_SUCCESS) return status;
		CubeGridShape shape = { g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch };
		status = check_triple_grid(fn, i, grid_count, format, shape, "coords", "coord_row_pitch");
		if (status != ASTCENC_SUCCESS) return status;
		size_t lod_row_pitch = g.lod_row_pitch;
		status = check_lod_buffer(fn, i, grid_count, g.lod, lod_row_pitch, g.out_x, g.out_y);
		if (status != ASTCENC_SUCCESS) return status;
		DecodeVolumeLaunch& l = launches[i];
		l.first_entry = g.first_entry; l.level_count = g.level_count;
		l.out_x = g.out_x; l.out_y = g.out_y;
		l.d_coords = g.coords;
		l.coord_row_pitch = shape.dir_row_pitch;
		l.d_lod = g.lod;
		l.lod_row_pitch = lod_row_pitch;
		l.lod_bias = g.lod_bias;
		l.d_out = g.out;
		l.row_pitch = shape.row_pitch; l.plane_pitch = shape.plane_pitch;
		if (!add_sample_tiles(fn, i, grid_count, g.out_x, g.out_y, tiles)) return ASTCENC_ERR_BAD_PARAM;
	}

	DecodeVolumeSampler smp;
	smp.filter = (uint32_t)sampler->filter;
	smp.address_x = (uint32_t)sampler->address_x; smp.address_y = (uint32_t)sampler->address_y; smp.address_z = (uint32_t)sampler->address_z;
	smp.mip_filter = (uint32_t)sampler->mip_filter;
	DecompressVolumeJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_volume);
}

} // extern "C"
