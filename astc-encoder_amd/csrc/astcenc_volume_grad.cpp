// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_volume_grad_device (include/astcenc_amd.h): the vector-Jacobian product of
// astcenc_amd_sample_volume_tensors_device with respect to the coordinates and the levels of detail -- the backward pass of a
// ray marcher, a deformation field or a neural field over volumes that stay compressed -- many grids per launch.  The format, the
// sampler, every entry and every grid are checked here as astcenc_volume.cpp checks them (sample_internal.h), then the buffers
// of the gradients as astcenc_lod_grad.cpp checks its own, all of it before anything is launched; the backend covers the tiles
// of all grids as one range of work items (backend_decompress_volume_grad).  The upstream gradients are data:
// none of them is an error.
// Product library only, like astcenc_volume.cpp.
#include "sample_internal.h"

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_volume_grad_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                    const astcenc_amd_tensor_format* format, const astcenc_amd_volume_sampler* sampler,
                                                    const astcenc_amd_volume_grad_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_volume_grad_device";
	if (grid_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !grids || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	DecodeTensorFormat fmt;
	DecodeLodSampler smp;
	std::vector<DecompressDeviceJob> jobs;
	// (every footprint is sampled here)
	astcenc_error status = check_lod_call(fn, ctx, entries, entry_count, format, sampler, true, fmt, smp, jobs);
	if (status != ASTCENC_SUCCESS) return status;

	// (a volume has no layer to pick: the launches' z stay 0)
	std::vector<DecodeLodGradLaunch> launches(grid_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < grid_count; i++)
	{
		const astcenc_amd_volume_grad_grid& g = grids[i];
		DecodeLodGradLaunch& l = launches[i];
		// (grad_out is read: the launch holds it where the forward call's holds its output)
		status = check_volume_grid(fn, i, grid_count, entries, entry_count, format, g, const_cast<void*>(g.grad_out), "grad_out", l.lod, tiles);
		if (status != ASTCENC_SUCCESS) return status;
		if (!g.grad_coords)
		{
			backend_log("%s: grid %u of %u: grad_coords is null", fn, i, grid_count);
			return ASTCENC_ERR_BAD_CONTEXT;
		}
		l.d_grad_coords = g.grad_coords;
		l.grad_coord_row_pitch = g.grad_coord_row_pitch;
		status = check_grad_buffer(fn, i, grid_count, "grad_coords", "grad_coord_row_pitch", g.grad_coords, l.grad_coord_row_pitch, 3, g.out_x, g.out_y);
		if (status != ASTCENC_SUCCESS) return status;
		l.d_grad_lod = g.grad_lod;
		l.grad_lod_row_pitch = g.grad_lod_row_pitch;
		status = check_grad_buffer(fn, i, grid_count, "grad_lod", "grad_lod_row_pitch", g.grad_lod, l.grad_lod_row_pitch, 1, g.out_x, g.out_y);
		if (status != ASTCENC_SUCCESS) return status;
	}

	DecompressLodGradJob job;
	memset(&job, 0, sizeof(job));
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	return run_windows_job(fn, ctx, jobs, hip_stream, job, backend_decompress_volume_grad);
}

} // extern "C"
