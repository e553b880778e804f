// SPDX-License-Identifier: Apache-2.0
// What the samplers' entry points share beyond regions_internal.h (astcenc_sample.cpp, astcenc_lod.cpp, astcenc_lod_grad.cpp,
// astcenc_cube.cpp, astcenc_volume.cpp, astcenc_volume_grad.cpp): the
// checks of the sampler's filter and address modes, of the footprint, of the entries' block counts, of a grid's points and their
// pairs or triples (check_sample_grid), of a chain and of the levels of detail, with the sample and lod calls' error codes and log
// lines; the checks of a call of the lod family as a whole (check_lod_call, check_lod_grid), to which the cube and volume calls
// bring their per-level check and the gradient those of its buffers.
// `fn` names the entry point in the log.
#pragma once
#include "regions_internal.h"

namespace astcd {

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

/* The context's footprint is 2D. */
inline astcenc_error check_sample_footprint(const char* fn, const astcenc_context* ctx)
{
	if (ctx->config.block_z <= 1) return ASTCENC_SUCCESS;
	backend_log("%s: the context's footprint %ux%ux%u is 3D: images of 2D footprints are sampled", fn, ctx->config.block_x, ctx->config.block_y,
	            ctx->config.block_z);
	return ASTCENC_ERR_BAD_PARAM;
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
 * interleaved layout).  A point has `per_point` floats: 2, the pairs of the sample and lod calls -- aligned to 8 bytes, an even
 * pitch of at least 2 out_x; or 3, the cube call's directions and the volume call's coordinates -- aligned to a float, any pitch
 * of at least 3 out_x.  `name` and `pitch_name` are the buffer's and its pitch's in the log. */
struct SampleGridShape {
	unsigned int out_x, out_y;
	const float* coords;
	size_t coord_row_pitch;
	void* out;
	size_t row_pitch, plane_pitch;
	unsigned int per_point = 2;
	const char* name = "coords";
	const char* pitch_name = "coord_row_pitch";
};

inline astcenc_error check_sample_grid(const char* fn, unsigned int i, unsigned int grid_count, const astcenc_amd_tensor_format* format, SampleGridShape& g,
                                       const char* out_name = "out")
{
	if (g.out_x == 0 || g.out_y == 0 || g.out_x > 65535 || g.out_y > 65535)
	{
		backend_log("%s: grid %u of %u: %u x %u points: either size is 1 to 65535", fn, i, grid_count, g.out_x, g.out_y);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const bool pairs = g.per_point == 2;
	const size_t tight = (size_t)g.per_point * g.out_x;
	if ((pairs && (g.coord_row_pitch & 1u) != 0) || (g.coord_row_pitch != 0 && g.coord_row_pitch < tight))
	{
		if (pairs) backend_log("%s: grid %u of %u: %s %zu: even and at least %zu floats", fn, i, grid_count, g.pitch_name, g.coord_row_pitch, tight);
		else backend_log("%s: grid %u of %u: %s %zu: at least %zu floats", fn, i, grid_count, g.pitch_name, g.coord_row_pitch, tight);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (the coordinates' extent in bytes fits 64 bits too: reported with the output's products)
	bool overflow = false;
	const size_t coord_row_pitch = g.coord_row_pitch ? g.coord_row_pitch : tight;
	(void)mul_safe(mul_safe(coord_row_pitch, g.out_y, overflow), sizeof(float), overflow);
	TensorPitches pitches = { g.row_pitch, 0, g.plane_pitch };
	const astcenc_error status = check_output_tensor(fn, "grid", i, grid_count, format, g.out_x, g.out_y, 0, pitches, g.out, overflow, !g.coords ? g.name : nullptr, out_name);
	if (status != ASTCENC_SUCCESS) return status;
	if (reinterpret_cast<uintptr_t>(g.coords) % (pairs ? 8 : 4) != 0)
	{
		if (pairs) backend_log("%s: grid %u of %u: %s %p is not aligned to a pair of floats (8 bytes)", fn, i, grid_count, g.name, static_cast<const void*>(g.coords));
		else backend_log("%s: grid %u of %u: %s %p is not aligned to a float (4 bytes)", fn, i, grid_count, g.name, static_cast<const void*>(g.coords));
		return ASTCENC_ERR_BAD_PARAM;
	}
	g.coord_row_pitch = coord_row_pitch;
	g.row_pitch = pitches.row;
	g.plane_pitch = pitches.plane;
	return ASTCENC_SUCCESS;
}

/* The mip filter between levels (astcenc_lod.cpp, astcenc_cube.cpp). */
inline astcenc_error check_mip_level_filter(const char* fn, int mip_filter)
{
	if (mip_filter == ASTCENC_AMD_MIP_NEAREST || mip_filter == ASTCENC_AMD_MIP_LINEAR) return ASTCENC_SUCCESS;
	backend_log("%s: sampler: mip_filter %d: not a mip filter", fn, mip_filter);
	return ASTCENC_ERR_BAD_PARAM;
}

/* The chain of grid i: 1 .. 32 levels, all of them entries of the call. */
inline astcenc_error check_lod_chain(const char* fn, unsigned int i, unsigned int grid_count, unsigned int first_entry, unsigned int level_count, unsigned int entry_count)
{
	if (level_count == 0 || level_count > 32)
	{
		backend_log("%s: grid %u of %u: %u levels: a chain has 1 to 32", fn, i, grid_count, level_count);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if ((unsigned long long)first_entry + level_count > entry_count)
	{
		backend_log("%s: grid %u of %u: levels are entries %u to %llu, the call has %u entries", fn, i, grid_count, first_entry,
		            (unsigned long long)first_entry + level_count - 1, entry_count);
		return ASTCENC_ERR_BAD_PARAM;
	}
	return ASTCENC_SUCCESS;
}

/* lod_bias and the lod buffer's pitch of grid i, before the grid's other buffers are looked at ... */
inline astcenc_error check_lod_pitch(const char* fn, unsigned int i, unsigned int grid_count, float lod_bias, size_t lod_row_pitch, unsigned int out_x)
{
	if (!std::isfinite(lod_bias))
	{
		backend_log("%s: grid %u of %u: lod_bias %g: not finite", fn, i, grid_count, (double)lod_bias);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (lod_row_pitch != 0 && lod_row_pitch < out_x)
	{
		backend_log("%s: grid %u of %u: lod_row_pitch %zu: at least %u floats", fn, i, grid_count, lod_row_pitch, out_x);
		return ASTCENC_ERR_BAD_PARAM;
	}
	return ASTCENC_SUCCESS;
}

/* ... and its extent and alignment after them; the pitch comes back resolved. */
inline astcenc_error check_lod_buffer(const char* fn, unsigned int i, unsigned int grid_count, const float* lod, size_t& lod_row_pitch, unsigned int out_x, unsigned int out_y)
{
	const size_t resolved = lod_row_pitch ? lod_row_pitch : out_x;
	bool overflow = false;
	(void)mul_safe(mul_safe(resolved, out_y, overflow), sizeof(float), overflow);
	if (overflow)
	{
		backend_log("%s: grid %u of %u: lod_row_pitch %zu: the levels of detail do not fit 64 bits", fn, i, grid_count, lod_row_pitch);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (reinterpret_cast<uintptr_t>(lod) % 4 != 0)
	{
		backend_log("%s: grid %u of %u: lod %p is not aligned to a float (4 bytes)", fn, i, grid_count, static_cast<const void*>(lod));
		return ASTCENC_ERR_BAD_PARAM;
	}
	lod_row_pitch = resolved;
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

/* The volume call's third address mode (astcenc_volume.cpp), after check_sample_modes has seen the other two. */
inline astcenc_error check_volume_address_z(const char* fn, int address_z)
{
	if (address_z >= ASTCENC_AMD_ADDRESS_CLAMP && address_z <= ASTCENC_AMD_ADDRESS_BORDER) return ASTCENC_SUCCESS;
	backend_log("%s: sampler: address mode %d along z: not an address mode", fn, address_z);
	return ASTCENC_ERR_BAD_PARAM;
}

/* check_sample_entries for any footprint (astcenc_volume.cpp): the blocks of an entry are counted in layers of block_z slices. */
inline astcenc_error check_volume_entries(const char* fn, astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                          std::vector<DecompressDeviceJob>& jobs)
{
	const astcenc_error entries_status = check_window_entries(fn, ctx, entries, entry_count, jobs);
	if (entries_status != ASTCENC_SUCCESS) return entries_status;
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		// (each factor is below 2^32 and the first product below 2^64; the second is formed only while it fits)
		const unsigned long long plane = (unsigned long long)((en.dim_x + ctx->config.block_x - 1) / ctx->config.block_x) *
		                                 ((en.dim_y + ctx->config.block_y - 1) / ctx->config.block_y);
		const unsigned long long layers = ((unsigned long long)en.dim_z + ctx->config.block_z - 1) / ctx->config.block_z;
		if (plane >= 0xFFFFFFFFull || plane * layers >= 0xFFFFFFFFull)
		{
			backend_log("%s: entry %u of %u: %llu x %llu blocks: an image of 2^32 - 1 blocks or more cannot be sampled", fn, e, entry_count, plane, layers);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}
	return ASTCENC_SUCCESS;
}

/* The sampler of a call of the lod family as the backend takes it; an address mode the call's sampler does not have is CLAMP. */
inline DecodeLodSampler lod_sampler_of(const astcenc_amd_lod_sampler& s)
{
	return { (uint32_t)s.filter, (uint32_t)s.address_x, (uint32_t)s.address_y, (uint32_t)s.mip_filter, ASTCENC_AMD_ADDRESS_CLAMP };
}
// (a cube has no address modes: its edges are its neighbours')
inline DecodeLodSampler lod_sampler_of(const astcenc_amd_cube_sampler& s)
{
	return { (uint32_t)s.filter, ASTCENC_AMD_ADDRESS_CLAMP, ASTCENC_AMD_ADDRESS_CLAMP, (uint32_t)s.mip_filter, ASTCENC_AMD_ADDRESS_CLAMP };
}
inline DecodeLodSampler lod_sampler_of(const astcenc_amd_volume_sampler& s)
{
	return { (uint32_t)s.filter, (uint32_t)s.address_x, (uint32_t)s.address_y, (uint32_t)s.mip_filter, (uint32_t)s.address_z };
}

/* What the lod call, its gradient, the cube call and the volume call check before their grids: the format, the sampler (the modes
 * it has: lod_sampler_of), the footprint -- 2D unless the call samples `any_footprint`, whose entries' blocks are counted in
 * layers -- and the entries; `fmt`, `smp` and `jobs` come back filled. */
template <class Sampler>
inline astcenc_error check_lod_call(const char* fn, astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                    const astcenc_amd_tensor_format* format, const Sampler* sampler, bool any_footprint, DecodeTensorFormat& fmt, DecodeLodSampler& smp,
                                    std::vector<DecompressDeviceJob>& jobs)
{
	astcenc_error status = check_tensor_format(fn, format);
	if (status != ASTCENC_SUCCESS) return status;
	if (!sampler)
	{
		backend_log("%s: sampler is null", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	smp = lod_sampler_of(*sampler);
	status = check_sample_modes(fn, (int)smp.filter, (int)smp.address_x, (int)smp.address_y);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_volume_address_z(fn, (int)smp.address_z);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_mip_level_filter(fn, (int)smp.mip_filter);
	if (status != ASTCENC_SUCCESS) return status;
	status = any_footprint ? ASTCENC_SUCCESS : check_sample_footprint(fn, ctx);
	if (status != ASTCENC_SUCCESS) return status;
	status = check_tensor_factors(fn, format, fmt);
	if (status != ASTCENC_SUCCESS) return status;
	return any_footprint ? check_volume_entries(fn, ctx, entries, entry_count, jobs) : check_sample_entries(fn, ctx, entries, entry_count, jobs);
}

/* ... and of grid i, any of the calls' grids: the chain, every level by level_check(entry, its index, level) -- which logs what it
 * rejects -- the levels of detail, the points, their coordinates as `points` has them (out_x .. coord_row_pitch, per_point and the
 * names; the rest is filled here) and the tensor `out` (a forward call's output or the gradient call's grad_out, named
 * `out_name` in the log); the launch comes back filled but for its z (the slice or the cube: the caller's) and the grid's tiles are added to `tiles`. */
template <class Grid, class LevelCheck>
inline astcenc_error check_lod_grid(const char* fn, unsigned int i, unsigned int grid_count, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                    const astcenc_amd_tensor_format* format, const Grid& g, SampleGridShape points, void* out, const char* out_name, LevelCheck level_check,
                                    DecodeLodLaunch& l, unsigned long long& tiles)
{
	astcenc_error status = check_lod_chain(fn, i, grid_count, g.first_entry, g.level_count, entry_count);
	if (status != ASTCENC_SUCCESS) return status;
	for (unsigned int lv = 0; lv < g.level_count; lv++)
	{
		status = level_check(entries[g.first_entry + lv], g.first_entry + lv, lv);
		if (status != ASTCENC_SUCCESS) return status;
	}
	status = check_lod_pitch(fn, i, grid_count, g.lod_bias, g.lod_row_pitch, g.out_x);
	if (status != ASTCENC_SUCCESS) return status;
	points.out = out; points.row_pitch = g.row_pitch; points.plane_pitch = g.plane_pitch;
	status = check_sample_grid(fn, i, grid_count, format, points, out_name);
	if (status != ASTCENC_SUCCESS) return status;
	size_t lod_row_pitch = g.lod_row_pitch;
	status = check_lod_buffer(fn, i, grid_count, g.lod, lod_row_pitch, g.out_x, g.out_y);
	if (status != ASTCENC_SUCCESS) return status;
	l.first_entry = g.first_entry; l.level_count = g.level_count;
	l.out_x = g.out_x; l.out_y = g.out_y;
	l.d_coords = points.coords;
	l.coord_row_pitch = points.coord_row_pitch;
	l.d_lod = g.lod;
	l.lod_row_pitch = lod_row_pitch;
	l.lod_bias = g.lod_bias;
	l.d_out = out;
	l.row_pitch = points.row_pitch; l.plane_pitch = points.plane_pitch;
	return add_sample_tiles(fn, i, grid_count, g.out_x, g.out_y, tiles) ? ASTCENC_SUCCESS : ASTCENC_ERR_BAD_PARAM;
}

/* The grid of the lod call or of its gradient (an astcenc_amd_lod_grid or an astcenc_amd_lod_grad_grid): pairs, and every level
 * holds the slice and is no larger than 65536 along x and y. */
template <class Grid>
inline astcenc_error check_lod_grid(const char* fn, unsigned int i, unsigned int grid_count, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                    const astcenc_amd_tensor_format* format, const Grid& g, void* out, const char* out_name, DecodeLodLaunch& l, unsigned long long& tiles)
{
	l.z = g.z;
	return check_lod_grid(fn, i, grid_count, entries, entry_count, format, g, { g.out_x, g.out_y, g.coords, g.coord_row_pitch }, out, out_name,
		[&](const astcenc_amd_image_set_entry& en, unsigned int entry, unsigned int lv)
		{
			if (g.z >= en.dim_z)
			{
				backend_log("%s: grid %u of %u: slice %u is not inside the %u x %u x %u image of entry %u (level %u)", fn, i, grid_count, g.z, en.dim_x, en.dim_y,
				            en.dim_z, entry, lv);
				return ASTCENC_ERR_BAD_PARAM;
			}
			// (a level coordinate is u W: within 2^30 for |u| <= 2^14)
			if (en.dim_x > 65536 || en.dim_y > 65536)
			{
				backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u texels: a level is at most 65536 along x and y", fn, i, grid_count, entry, lv, en.dim_x,
				            en.dim_y);
				return ASTCENC_ERR_BAD_PARAM;
			}
			return ASTCENC_SUCCESS;
		}, l, tiles);
}

/* The grid of the volume call or of its gradient (an astcenc_amd_volume_grid or an astcenc_amd_volume_grad_grid): triples, no
 * slice to pick (the launch's z stays 0), and every level is no larger than 65536 along x, y and z. */
template <class Grid>
inline astcenc_error check_volume_grid(const char* fn, unsigned int i, unsigned int grid_count, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                       const astcenc_amd_tensor_format* format, const Grid& g, void* out, const char* out_name, DecodeLodLaunch& l, unsigned long long& tiles)
{
	SampleGridShape points = { g.out_x, g.out_y, g.coords, g.coord_row_pitch };
	points.per_point = 3;
	return check_lod_grid(fn, i, grid_count, entries, entry_count, format, g, points, out, out_name,
		[&](const astcenc_amd_image_set_entry& en, unsigned int entry, unsigned int lv)
		{
			// (a level coordinate is u W: within 2^30 for |u| <= 2^14)
			if (en.dim_x <= 65536 && en.dim_y <= 65536 && en.dim_z <= 65536) return ASTCENC_SUCCESS;
			backend_log("%s: grid %u of %u: entry %u (level %u) is %u x %u x %u texels: a level is at most 65536 along x, y and z", fn, i, grid_count, entry, lv, en.dim_x,
			            en.dim_y, en.dim_z);
			return ASTCENC_ERR_BAD_PARAM;
		}, l, tiles);
}

/* A buffer of a gradient call that is written, `name` with its pitch `pitch_name`: `per_point` floats a point (2: the lod
 * gradient's grad_coords, aligned to 8 bytes, an even pitch; 3: the volume gradient's, aligned to 4 bytes, any pitch; 1: grad_lod,
 * aligned to 4 bytes); the pitch comes back resolved. */
inline astcenc_error check_grad_buffer(const char* fn, unsigned int i, unsigned int grid_count, const char* name, const char* pitch_name, const float* buffer,
                                       size_t& row_pitch, unsigned int per_point, unsigned int out_x, unsigned int out_y)
{
	const unsigned int align = per_point == 2 ? 8u : 4u;
	const size_t tight = (size_t)per_point * out_x;
	if ((per_point == 2 && (row_pitch & 1u) != 0) || (row_pitch != 0 && row_pitch < tight))
	{
		backend_log("%s: grid %u of %u: %s %zu: %sat least %zu floats", fn, i, grid_count, pitch_name, row_pitch, per_point == 2 ? "even and " : "", tight);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const size_t resolved = row_pitch ? row_pitch : tight;
	bool overflow = false;
	(void)mul_safe(mul_safe(resolved, out_y, overflow), sizeof(float), overflow);
	if (overflow)
	{
		backend_log("%s: grid %u of %u: %s %zu: the gradients do not fit 64 bits", fn, i, grid_count, pitch_name, row_pitch);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (reinterpret_cast<uintptr_t>(buffer) % align != 0)
	{
		backend_log("%s: grid %u of %u: %s %p is not aligned to %u bytes", fn, i, grid_count, name, static_cast<const void*>(buffer), align);
		return ASTCENC_ERR_BAD_PARAM;
	}
	row_pitch = resolved;
	return ASTCENC_SUCCESS;
}

} // namespace astcd
