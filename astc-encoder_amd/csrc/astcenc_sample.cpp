// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_sample_tensors_device (include/astcenc_amd.h): device-resident compressed images sampled at buffers of coordinates
// -- the UV buffer of a rasteriser, a warp field, a rotated crop -- and written as tensors, many grids per launch.  The format,
// the sampler, every entry and every grid are checked here, all of them before anything is launched; the backend then covers the
// tiles of all grids as one range of work items (backend_decompress_sample).  The coordinates themselves are
// data: none of them is an error.
// Product library only, like astcenc_scaled.cpp.
#include "regions_internal.h"

#include <cmath>

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_sample_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                const astcenc_amd_tensor_format* format, const astcenc_amd_sampler* sampler,
                                                const astcenc_amd_sample_grid* grids, unsigned int grid_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_sample_tensors_device";
	if (grid_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !grids || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
	if (!format)
	{
		backend_log("%s: format is null", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if ((int)format->type < ASTCENC_AMD_TENSOR_F32 || (int)format->type > ASTCENC_AMD_TENSOR_BF16 ||
	    (int)format->layout < ASTCENC_AMD_TENSOR_PLANAR || (int)format->layout > ASTCENC_AMD_TENSOR_INTERLEAVED)
	{
		backend_log("%s: format: type %d, layout %d: not a tensor type / layout", fn, (int)format->type, (int)format->layout);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (format->channels < 1 || format->channels > 4)
	{
		backend_log("%s: format: %u channels: 1 to 4 can be had", fn, format->channels);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (!sampler)
	{
		backend_log("%s: sampler is null", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if ((int)sampler->filter != ASTCENC_AMD_SAMPLE_NEAREST && (int)sampler->filter != ASTCENC_AMD_SAMPLE_BILINEAR)
	{
		backend_log("%s: sampler: filter %d: not a sample filter", fn, (int)sampler->filter);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if ((int)sampler->address_x < ASTCENC_AMD_ADDRESS_CLAMP || (int)sampler->address_x > ASTCENC_AMD_ADDRESS_BORDER ||
	    (int)sampler->address_y < ASTCENC_AMD_ADDRESS_CLAMP || (int)sampler->address_y > ASTCENC_AMD_ADDRESS_BORDER)
	{
		backend_log("%s: sampler: address modes %d, %d: not address modes", fn, (int)sampler->address_x, (int)sampler->address_y);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (ctx->config.block_z > 1)
	{
		backend_log("%s: the context's footprint %ux%ux%u is 3D: images of 2D footprints are sampled", fn, ctx->config.block_x, ctx->config.block_y,
		            ctx->config.block_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	DecodeTensorFormat fmt;
	memset(&fmt, 0, sizeof(fmt));
	fmt.type = (uint32_t)format->type; fmt.layout = (uint32_t)format->layout; fmt.channels = format->channels;
	for (unsigned int c = 0; c < format->channels; c++)
	{
		if (!std::isfinite(format->scale[c]) || !std::isfinite(format->bias[c]))
		{
			backend_log("%s: format: scale %g, bias %g of channel %u: not finite", fn, (double)format->scale[c], (double)format->bias[c], c);
			return ASTCENC_ERR_BAD_PARAM;
		}
		fmt.scale[c] = format->scale[c]; fmt.bias[c] = format->bias[c];
	}
	const bool planar = format->layout == ASTCENC_AMD_TENSOR_PLANAR;
	const size_t element = format->type == ASTCENC_AMD_TENSOR_F32 ? 4 : 2;

	std::vector<DecompressDeviceJob> jobs;
	const astcenc_error entries_status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (entries_status != ASTCENC_SUCCESS) return entries_status;
	// (a tap's block is a 32-bit index in the kernel)
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		const unsigned long long blocks = (unsigned long long)((en.dim_x + ctx->config.block_x - 1) / ctx->config.block_x) *
		                                  ((en.dim_y + ctx->config.block_y - 1) / ctx->config.block_y) * en.dim_z;
		if (blocks >= 0xFFFFFFFFull)
		{
			backend_log("%s: entry %u of %u: %llu blocks: an image of 2^32 - 1 blocks or more cannot be sampled", fn, e, entry_count, blocks);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}

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
		if (g.out_x == 0 || g.out_y == 0 || g.out_x > 65535 || g.out_y > 65535)
		{
			backend_log("%s: grid %u of %u: %u x %u points: either size is 1 to 65535", fn, i, grid_count, g.out_x, g.out_y);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if ((g.coord_row_pitch & 1u) != 0 || (g.coord_row_pitch != 0 && g.coord_row_pitch < 2u * (size_t)g.out_x))
		{
			backend_log("%s: grid %u of %u: coord_row_pitch %zu: even and at least %zu floats", fn, i, grid_count, g.coord_row_pitch, 2u * (size_t)g.out_x);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// pitches in elements, every product in 64 bits: the tensor's extent in bytes must fit them too
		bool overflow = false;
		const size_t tight_row = mul_safe(g.out_x, planar ? 1 : format->channels, overflow);
		const size_t row_pitch = g.row_pitch ? g.row_pitch : tight_row;
		const size_t tight_plane = mul_safe(row_pitch, g.out_y, overflow);
		const size_t plane_pitch = g.plane_pitch ? g.plane_pitch : tight_plane;
		(void)mul_safe(planar ? mul_safe(plane_pitch, format->channels, overflow) : tight_plane, element, overflow);
		const size_t coord_row_pitch = g.coord_row_pitch ? g.coord_row_pitch : 2u * (size_t)g.out_x;
		(void)mul_safe(mul_safe(coord_row_pitch, g.out_y, overflow), sizeof(float), overflow);
		if (overflow || row_pitch < tight_row || (planar && plane_pitch < tight_plane))
		{
			backend_log("%s: grid %u of %u: row_pitch %zu, plane_pitch %zu: the output needs at least %zu and %zu elements", fn, i, grid_count, g.row_pitch,
			            g.plane_pitch, tight_row, tight_plane);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (!planar && g.plane_pitch != 0)
		{
			backend_log("%s: grid %u of %u: plane_pitch %zu: the interleaved layout has no planes", fn, i, grid_count, g.plane_pitch);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// (a null buffer: what the other device calls return for one)
		if (!g.out || !g.coords)
		{
			backend_log("%s: grid %u of %u: %s is null", fn, i, grid_count, !g.out ? "out" : "coords");
			return ASTCENC_ERR_BAD_CONTEXT;
		}
		if (reinterpret_cast<uintptr_t>(g.out) % element != 0)
		{
			backend_log("%s: grid %u of %u: out %p is not aligned to the element size %zu", fn, i, grid_count, g.out, element);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (reinterpret_cast<uintptr_t>(g.coords) % 8 != 0)
		{
			backend_log("%s: grid %u of %u: coords %p is not aligned to a pair of floats (8 bytes)", fn, i, grid_count, static_cast<const void*>(g.coords));
			return ASTCENC_ERR_BAD_PARAM;
		}
		DecodeSampleLaunch& l = launches[i];
		l.entry = g.entry;
		l.z = g.z;
		l.out_x = g.out_x; l.out_y = g.out_y;
		l.d_coords = g.coords;
		l.coord_row_pitch = coord_row_pitch;
		l.d_out = g.out;
		l.row_pitch = row_pitch; l.plane_pitch = planar ? plane_pitch : 0;
		tiles += astc_decode_sample_tiles(g.out_x, g.out_y);
		if (tiles > 0xFFFFFFFFull)
		{
			backend_log("%s: grid %u of %u: more than 2^32 - 1 tiles of points in all", fn, i, grid_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}

	DecodeSampler smp;
	smp.filter = (uint32_t)sampler->filter; smp.address_x = (uint32_t)sampler->address_x; smp.address_y = (uint32_t)sampler->address_y;
	DecompressSampleJob job;
	memset(&job, 0, sizeof(job));
	job.entries = jobs.data();
	job.entry_count = entry_count;
	job.format = &fmt;
	job.sampler = &smp;
	job.grids = launches.data();
	job.grid_count = grid_count;
	job.stream = hip_stream;
	const astcenc_error status = windows_rc_to_error(backend_decompress_sample(ctx->backend, job));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: a buffer or hip_stream is not on the device of entry 0's blocks", fn);
	return status;
}

} // extern "C"
