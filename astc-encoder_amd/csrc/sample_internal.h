// SPDX-License-Identifier: Apache-2.0
// What the two samplers' entry points share (astcenc_sample.cpp, astcenc_lod.cpp): the checks of the format, of the sampler's
// filter and address modes, of the entries' block counts and of a grid's points, coordinates and output, with the sample call's
// error codes and log lines.  `fn` names the entry point in the log.
#pragma once
#include "regions_internal.h"

#include <cmath>

namespace astcd {

/* The format's type, layout and channels. */
inline astcenc_error check_sample_format(const char* fn, const astcenc_amd_tensor_format* format)
{
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
	return ASTCENC_SUCCESS;
}

/* The sampler's filter and address modes. */
inline astcenc_error check_sample_modes(const char* fn, int filter, int address_x, int address_y)
{
	if (filter != ASTCENC_AMD_SAMPLE_NEAREST && filter != ASTCENC_AMD_SAMPLE_BILINEAR)
	{
		backend_log("%s: sampler: filter %d: not a sample filter", fn, filter);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (address_x < ASTCENC_AMD_ADDRESS_CLAMP || address_x > ASTCENC_AMD_ADDRESS_BORDER || address_y < ASTCENC_AMD_ADDRESS_CLAMP || address_y > ASTCENC_AMD_ADDRESS_BORDER)
	{
		backend_log("%s: sampler: address modes %d, %d: not address modes", fn, address_x, address_y);
		return ASTCENC_ERR_BAD_PARAM;
	}
	return ASTCENC_SUCCESS;
}

/* The context's footprint is 2D and the (checked) format's factors are finite; fmt: the format for the backend. */
inline astcenc_error check_sample_factors(const char* fn, const astcenc_context* ctx, const astcenc_amd_tensor_format* format, DecodeTensorFormat& fmt)
{
	if (ctx->config.block_z > 1)
	{
		backend_log("%s: the context's footprint %ux%ux%u is 3D: images of 2D footprints are sampled", fn, ctx->config.block_x, ctx->config.block_y,
		            ctx->config.block_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
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
	return ASTCENC_SUCCESS;
}

/* Every entry as the windowed decoders check it, and no entry of 2^32 - 1 blocks or more (a tap's block is a 32-bit index in the
 * kernels). */
inline astcenc_error check_sample_entries(const char* fn, astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                          std::vector<DecompressDeviceJob>& jobs)
{
	const astcenc_error entries_status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (entries_status != ASTCENC_SUCCESS) return entries_status;
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
	return ASTCENC_SUCCESS;
}

/* The points, the coordinates and the output of grid i of grid_count; the pitches come back resolved (plane_pitch 0 for the
 * interleaved layout). */
struct SampleGridShape {
	unsigned int out_x, out_y;
	const float* coords;
	size_t coord_row_pitch;
	void* out;
	size_t row_pitch, plane_pitch;
};

inline astcenc_error check_sample_grid(const char* fn, unsigned int i, unsigned int grid_count, const astcenc_amd_tensor_format* format, SampleGridShape& g)
{
	const bool planar = format->layout == ASTCENC_AMD_TENSOR_PLANAR;
	const size_t element = format->type == ASTCENC_AMD_TENSOR_F32 ? 4 : 2;
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
	g.coord_row_pitch = coord_row_pitch;
	g.row_pitch = row_pitch;
	g.plane_pitch = planar ? plane_pitch : 0;
	return ASTCENC_SUCCESS;
}

/* The running sum of the call's tiles after grid i; false (logged) past 2^32 - 1. */
inline bool add_sample_tiles(const char* fn, unsigned int i, unsigned int grid_count, unsigned int out_x, unsigned int out_y, unsigned long long& tiles)
{
	tiles += astc_decode_sample_tiles(out_x, out_y);
	if (tiles <= 0xFFFFFFFFull) return true;
	backend_log("%s: grid %u of %u: more than 2^32 - 1 tiles of points in all", fn, i, grid_count);
	return false;
}

} // namespace astcd
