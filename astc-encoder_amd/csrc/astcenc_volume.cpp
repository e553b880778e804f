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
	DecodeTensorFormat fmt;
	DecodeLodSampler smp;
	std::vector<DecompressDeviceJob> jobs;
	// (every footprint is sampled here)
	astcenc_error status = check_lod_call(fn, ctx, entries, entry_count, format, sampler, true, fmt, smp, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	// (a volume has no layer to pick: the launches' stay 0)
	std::vector<DecodeLodLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		status = check_volume_grid(fn, i, grid_count, entries, entry_count, format, grids[i], grids[i].out, "out", launches[i], tiles);
		if (status != ASTCENC_SUCCESS) return status;
	}

	DecompressLodJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_volume);
}

} // extern "C"
