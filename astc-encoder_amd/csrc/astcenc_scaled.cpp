// SPDX-License-Identifier: Apache-2.0
// astcenc_amd_decompress_scaled_tensors_device (include/astcenc_amd.h): windows of device-resident compressed images resampled
// to a size of their own and written as tensors -- the random resized crop of a training loader -- many per launch.  The format,
// the filter, every entry and every region are checked here, all of them before anything is launched; the backend then covers
// the output tiles of all regions as one range of work items (backend_decompress_scaled).
// Product library only, like astcenc_tensors.cpp.
#include "regions_internal.h"

#include <cmath>

using namespace astcd;

extern "C" {

astcenc_error astcenc_amd_decompress_scaled_tensors_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                           const astcenc_amd_tensor_format* format, astcenc_amd_window_filter filter,
                                                           const astcenc_amd_scaled_region* regions, unsigned int region_count, void* hip_stream)
{
	const char* fn = "astcenc_amd_decompress_scaled_tensors_device";
	if (region_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !regions || (!entries && entry_count != 0)) return ASTCENC_ERR_BAD_PARAM;
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
	if ((int)filter != ASTCENC_AMD_WINDOW_BILINEAR && (int)filter != ASTCENC_AMD_WINDOW_BOX)
	{
		backend_log("%s: filter %d: not a window filter", fn, (int)filter);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (ctx->config.block_z > 1)
	{
		backend_log("%s: the context's footprint %ux%ux%u is 3D: windows of 2D footprints are resampled", fn, ctx->config.block_x, ctx->config.block_y,
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

	std::vector<DecodeScaledLaunch> launches(region_count);
	unsigned long long tiles = 0;
	for (unsigned int i = 0; i < region_count; i++)
	{
		const astcenc_amd_scaled_region& r = regions[i];
		// (entry, zero window sizes, the window and its slice inside the image)
		const astcenc_error window_status = check_window(fn, i, region_count, entries, entry_count, r.entry, r.x, r.y, r.z, r.size_x, r.size_y, 1);
		if (window_status != ASTCENC_SUCCESS) return window_status;
		if (r.out_x == 0 || r.out_y == 0 || r.size_x > 65535 || r.size_y > 65535 || r.out_x > 65535 || r.out_y > 65535)
		{
			backend_log("%s: region %u of %u: window %u x %u to %u x %u: every size is 1 to 65535", fn, i, region_count, r.size_x, r.size_y, r.out_x, r.out_y);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (r.flags & ~(ASTCENC_AMD_TENSOR_FLIP_X | ASTCENC_AMD_TENSOR_FLIP_Y))
		{
			backend_log("%s: region %u of %u: flags 0x%x: unknown bits", fn, i, region_count, r.flags);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// pitches in elements, every product in 64 bits: the tensor's extent in bytes must fit them too
		bool overflow = false;
		const size_t tight_row = mul_safe(r.out_x, planar ? 1 : format->channels, overflow);
		const size_t row_pitch = r.row_pitch ? r.row_pitch : tight_row;
		const size_t tight_plane = mul_safe(row_pitch, r.out_y, overflow);
		const size_t plane_pitch = r.plane_pitch ? r.plane_pitch : tight_plane;
		(void)mul_safe(planar ? mul_safe(plane_pitch, format->channels, overflow) : tight_plane, element, overflow);
		if (overflow || row_pitch < tight_row || (planar && plane_pitch < tight_plane))
		{
			backend_log("%s: region %u of %u: row_pitch %zu, plane_pitch %zu: the output needs at least %zu and %zu elements", fn, i, region_count, r.row_pitch,
			            r.plane_pitch, tight_row, tight_plane);
			return ASTCENC_ERR_BAD_PARAM;
		}
		if (!planar && r.plane_pitch != 0)
		{
			backend_log("%s: region %u of %u: plane_pitch %zu: the interleaved layout has no planes", fn, i, region_count, r.plane_pitch);
			return ASTCENC_ERR_BAD_PARAM;
		}
		// (a null buffer: what the other device calls return for one)
		if (!r.out)
		{
			backend_log("%s: region %u of %u: out is null", fn, i, region_count);
			return ASTCENC_ERR_BAD_CONTEXT;
		}
		if (reinterpret_cast<uintptr_t>(r.out) % element != 0)
		{
			backend_log("%s: region %u of %u: out %p is not aligned to the element size %zu", fn, i, region_count, r.out, element);
			return ASTCENC_ERR_BAD_PARAM;
		}
		DecodeScaledLaunch& l = launches[i];
		l.entry = r.entry;
		l.x = r.x; l.y = r.y; l.z = r.z;
		l.size_x = r.size_x; l.size_y = r.size_y;
		l.out_x = r.out_x; l.out_y = r.out_y;
		l.flags = r.flags;
		l.d_out = r.out;
		l.row_pitch = row_pitch; l.plane_pitch = planar ? plane_pitch : 0;
		tiles += astc_decode_scaled_tiles(l, (uint32_t)entries[r.entry].data_type, ctx->config.block_x, ctx->config.block_y);
		if (tiles > 0xFFFFFFFFull)
		{
			backend_log("%s: region %u of %u: more than 2^32 - 1 output tiles in all", fn, i, region_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}

	DecompressScaledJob job;
	memset(&job, 0, sizeof(job));
	job.entries = jobs.data();
	job.entry_count = entry_count;
	job.format = &fmt;
	job.filter = (uint32_t)filter;
	job.regions = launches.data();
	job.region_count = region_count;
	job.stream = hip_stream;
	const astcenc_error status = windows_rc_to_error(backend_decompress_scaled(ctx->backend, job));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: a buffer or hip_stream is not on the device of entry 0's blocks", fn);
	return status;
}

} // extern "C"
