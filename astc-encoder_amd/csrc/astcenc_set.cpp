// SPDX-License-Identifier: Apache-2.0
// The image-set entry points (include/astcenc_amd.h): many device-resident images through one chain of kernel launches.
// Every entry is checked exactly as the single-image entry point checks its image, all of them before anything is launched;
// the backend then compresses (decompresses) the blocks of all entries as one range (backend_compress_set).
// Product library only: the sequential build of oracle/emu has no backend_*_set.
// The mip chain entry points live here too: a compressed chain is an image set of one entry per level, its generation queued
// ahead of the set's launches (backend_compress_set with CompressSetJob::generate; the filter: mip_filter.h, the windowed
// filters of the _filtered_ calls: mip_resample.h, the weighting of the _weighted_ calls: mip_weighted.h, the post-passes of the
// _ex_ calls: mip_post.h).  Every mip call is one path: the calls without options, a filter or a weighting pass null ones.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"
#include "mip_resize.h"

#include <cstring>
#include <vector>

using namespace astcd;

static astcenc_error rc_to_error(int rc)
{
	return rc == 0 ? ASTCENC_SUCCESS : rc == 1 ? ASTCENC_ERR_OUT_OF_MEM : rc == 3 ? ASTCENC_ERR_BAD_PARAM : ASTCENC_ERR_BAD_CONTEXT;
}

/* The blocks of all entries are counted by one 32-bit index (the kernels' block and run numbers). */
static bool set_fits_32_bits(const std::vector<size_t>& blocks)
{
	size_t total = 0;
	for (size_t n : blocks)
	{
		total += n;
		if (total > 0xFFFFFFFFull) return false;
	}
	return true;
}

/* Checks every entry of a compression set and fills its job (entry_internal.h). */
astcenc_error astcd::check_compress_set(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                        std::vector<CompressJob>& jobs, size_t& total)
{
	const bool alpha_scale = ctx->config.a_scale_radius != 0 && ctx->config.block_z <= 1;
	jobs.resize(entry_count);
	std::vector<size_t> blocks(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		astcenc_error status = check_compress_args(ctx, en.dim_x, en.dim_y, en.dim_z, &en.swizzle, en.blocks_len, 0, blocks[e]);
		// (a null buffer: what astcenc_amd_compress_volume_device returns for it, before it launches anything)
		if (status == ASTCENC_SUCCESS && (!en.image || !en.blocks)) status = ASTCENC_ERR_BAD_CONTEXT;
		if (status != ASTCENC_SUCCESS)
		{
			backend_log("image set entry %u of %u: %s", e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		CompressJob& job = jobs[e];
		memset(&job, 0, sizeof(job));
		job.device_data = en.image;
		job.dim_x = en.dim_x; job.dim_y = en.dim_y; job.dim_z = en.dim_z;
		job.data_type = (uint32_t)en.data_type;
		job.swz[0] = en.swizzle.r; job.swz[1] = en.swizzle.g; job.swz[2] = en.swizzle.b; job.swz[3] = en.swizzle.a;
		job.device_out = static_cast<uint8_t*>(en.blocks);
		job.a_scale_radius = alpha_scale ? ctx->config.a_scale_radius : 0u;
		// (the default of astcenc_amd_compress_volume_device: every slice from its own data)
		job.fast_load_slice0 = ctx->per_slice_fast_load == 0 ? 1u : 0u;
	}
	if (!set_fits_32_bits(blocks))
	{
		backend_log("image set of %u entries: more than 2^32 - 1 blocks", entry_count);
		return ASTCENC_ERR_BAD_PARAM;
	}
	total = 0;
	for (size_t n : blocks) total += n;
	return ASTCENC_SUCCESS;
}

/* Checks every entry of a compression set and launches it; the generation of a mip chain (`generate`, may be null) is queued
 * ahead of the set's launches on the same stream.  Nothing is launched unless every check passes. */
static astcenc_error compress_set(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                  void* hip_stream, float* kernel_ms, const MipChainJob* generate)
{
	std::vector<CompressJob> jobs;
	size_t total;
	const astcenc_error status = check_compress_set(ctx, entries, entry_count, jobs, total);
	if (status != ASTCENC_SUCCESS) return status;

	// cancel: the rules of astcenc_amd_compress_volume_device (a thread_count == 1 context starts clean, a multi-thread
	// context's cancel is sticky until astcenc_compress_reset)
	if (ctx->thread_count == 1) ctx->cancel_flag.store(0);
	CompressSetJob set;
	memset(&set, 0, sizeof(set));
	set.entries = jobs.data();
	set.count = entry_count;
	set.stream = hip_stream;
	set.kernel_ms = kernel_ms;
	set.cancel_flag = &ctx->cancel_flag;
	set.progress = ctx->config.progress_callback;
	set.generate = generate;
	return rc_to_error(backend_compress_set(ctx->backend, set));
}

extern "C" {

astcenc_error astcenc_amd_compress_images_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                 void* hip_stream, float* kernel_ms)
{
	if (entry_count == 0)
	{
		if (kernel_ms) *kernel_ms = 0.0f;
		return ASTCENC_SUCCESS;
	}
	if (!ctx || !entries) return ASTCENC_ERR_BAD_PARAM;
	return compress_set(ctx, entries, entry_count, hip_stream, kernel_ms, nullptr);
}

astcenc_error astcenc_amd_decompress_images_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                   void* hip_stream)
{
	if (entry_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !entries) return ASTCENC_ERR_BAD_PARAM;
	std::vector<DecompressDeviceJob> jobs(entry_count);
	std::vector<size_t> blocks(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		const astcenc_error status = check_decompress_device_args(ctx, en.blocks, en.blocks_len, en.image, en.dim_x, en.dim_y, en.dim_z, &en.swizzle);
		if (status != ASTCENC_SUCCESS)
		{
			backend_log("image set entry %u of %u: %s", e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		blocks[e] = block_count_axis(en.dim_x, ctx->config.block_x) * block_count_axis(en.dim_y, ctx->config.block_y) *
		            block_count_axis(en.dim_z, ctx->config.block_z);
		DecompressDeviceJob& job = jobs[e];
		memset(&job, 0, sizeof(job));
		job.device_blocks = static_cast<const uint8_t*>(en.blocks);
		job.device_image = en.image;
		job.dim_x = en.dim_x; job.dim_y = en.dim_y; job.dim_z = en.dim_z;
		job.data_type = (uint32_t)en.data_type;
		job.swz[0] = en.swizzle.r; job.swz[1] = en.swizzle.g; job.swz[2] = en.swizzle.b; job.swz[3] = en.swizzle.a;
	}
	if (!set_fits_32_bits(blocks))
	{
		backend_log("image set of %u entries: more than 2^32 - 1 blocks", entry_count);
		return ASTCENC_ERR_BAD_PARAM;
	}
	DecompressSetJob set;
	memset(&set, 0, sizeof(set));
	set.entries = jobs.data();
	set.count = entry_count;
	set.stream = hip_stream;
	return rc_to_error(backend_decompress_set(ctx->backend, set));
}

/* Mip chains (include/astcenc_amd.h): the layout is host arithmetic; generation and compression check everything first.  A 2D
 * chain is the VOLUME of depth 1: that kind takes the 3D footprints the 2D calls take, and at depth 1 it has the 2D layout and
 * makes its levels with the 2D kernels (kernel_mips.hip). */
astcenc_error astcenc_amd_mip_chain_volume_layout(const astcenc_config* config, unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                                  astcenc_amd_mip_kind kind, astcenc_type data_type, unsigned int level_count,
                                                  struct astcenc_amd_mip_chain_volume_layout* layout)
{
	if (!config || !layout) return ASTCENC_ERR_BAD_PARAM;
	memset(layout, 0, sizeof(*layout));
	if (dim_x == 0 || dim_y == 0 || dim_z == 0 || config->block_x == 0 || config->block_y == 0 || config->block_z == 0) return ASTCENC_ERR_BAD_PARAM;
	if ((int)data_type < ASTCENC_TYPE_U8 || (int)data_type > ASTCENC_TYPE_F32) return ASTCENC_ERR_BAD_PARAM;
	if (kind != ASTCENC_AMD_MIP_ARRAY && kind != ASTCENC_AMD_MIP_VOLUME) return ASTCENC_ERR_BAD_PARAM;
	// (an array's blocks must not span layers)
	if (kind == ASTCENC_AMD_MIP_ARRAY && config->block_z > 1) return ASTCENC_ERR_BAD_PARAM;
	const bool volume = kind == ASTCENC_AMD_MIP_VOLUME;
	const unsigned int full = volume ? mip_full_levels_3d(dim_x, dim_y, dim_z) : mip_full_levels(dim_x, dim_y);
	if (level_count > full) return ASTCENC_ERR_BAD_PARAM;
	const unsigned int n = level_count == 0 ? full : level_count;
	const size_t texel_bytes = data_type == ASTCENC_TYPE_U8 ? 4 : data_type == ASTCENC_TYPE_F16 ? 8 : 16;
	size_t texels = 0, blocks = 0;
	bool overflow = false;
	for (unsigned int i = 0; i < n; i++)
	{
		const unsigned int dx = mip_level_dim(dim_x, i), dy = mip_level_dim(dim_y, i), dz = volume ? mip_level_dim(dim_z, i) : dim_z;
		layout->dim_x[i] = dx;
		layout->dim_y[i] = dy;
		layout->dim_z[i] = dz;
		layout->blocks_offset[i] = blocks;
		const size_t level_blocks = mul_safe(mul_safe(block_count_axis(dx, config->block_x), block_count_axis(dy, config->block_y), overflow),
		                                     block_count_axis(dz, config->block_z), overflow);
		const size_t level_block_bytes = mul_safe(level_blocks, 16, overflow);
		overflow = overflow || blocks + level_block_bytes < blocks;
		blocks += level_block_bytes;
		// (level 0 is the caller's: its bytes must exist, but it takes no room in device_levels)
		const size_t level_bytes = mul_safe(mul_safe(mul_safe(dx, dy, overflow), dz, overflow), texel_bytes, overflow);
		if (i == 0) continue;
		const size_t at = (texels + MIP_LEVEL_ALIGN - 1) & ~(size_t)(MIP_LEVEL_ALIGN - 1);
		overflow = overflow || at < texels || at + level_bytes < at;
		layout->texels_offset[i] = at;
		texels = at + level_bytes;
	}
	if (overflow)
	{
		memset(layout, 0, sizeof(*layout));
		return ASTCENC_ERR_BAD_PARAM;
	}
	layout->level_count = n;
	layout->texels_len = texels;
	layout->blocks_len = blocks;
	return ASTCENC_SUCCESS;
}

static astcenc_error check_mip_volume_args(const char* fn, astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                           unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type, unsigned int level_count,
                                           void* device_levels, size_t levels_len, void* hip_stream,
                                           struct astcenc_amd_mip_chain_volume_layout& layout, MipChainJob& gen)
{
	astcenc_error status = astcenc_amd_mip_chain_volume_layout(&ctx->config, dim_x, dim_y, dim_z, kind, data_type, level_count, &layout);
	if (status != ASTCENC_SUCCESS)
	{
		const char* why = "bad image";
		if (kind != ASTCENC_AMD_MIP_ARRAY && kind != ASTCENC_AMD_MIP_VOLUME) why = "kind is neither ASTCENC_AMD_MIP_ARRAY nor ASTCENC_AMD_MIP_VOLUME";
		else if (kind == ASTCENC_AMD_MIP_ARRAY && ctx->config.block_z > 1) why = "kind ASTCENC_AMD_MIP_ARRAY with a 3D footprint";
		else if (dim_x && dim_y && dim_z &&
		         level_count > (kind == ASTCENC_AMD_MIP_VOLUME ? mip_full_levels_3d(dim_x, dim_y, dim_z) : mip_full_levels(dim_x, dim_y)))
			why = "level_count exceeds the full chain";
		else if (dim_x && dim_y && dim_z && (int)data_type >= ASTCENC_TYPE_U8 && (int)data_type <= ASTCENC_TYPE_F32)
			why = "the chain's bytes overflow size_t";
		backend_log("%s: dim_x %u, dim_y %u, dim_z %u, kind %d, data_type %d, level_count %u: %s", fn, dim_x, dim_y, dim_z, (int)kind,
		            (int)data_type, level_count, why);
		return status;
	}
	// (a null buffer: what astcenc_amd_compress_image_device returns for one)
	if (!device_image) { backend_log("%s: device_image is null", fn); return ASTCENC_ERR_BAD_CONTEXT; }
	if (layout.level_count > 1 && !device_levels) { backend_log("%s: device_levels is null", fn); return ASTCENC_ERR_BAD_CONTEXT; }
	if (levels_len < layout.texels_len)
	{
		backend_log("%s: levels_len %zu, the chain needs %zu", fn, levels_len, layout.texels_len);
		return ASTCENC_ERR_OUT_OF_MEM;
	}
	memset(&gen, 0, sizeof(gen));
	gen.device_image = device_image;
	gen.dim_x = dim_x; gen.dim_y = dim_y; gen.dim_z = dim_z; gen.kind = (uint32_t)kind;
	gen.data_type = (uint32_t)data_type; gen.level_count = layout.level_count;
	gen.srgb = ctx->config.profile == ASTCENC_PRF_LDR_SRGB ? 1u : 0u;
	gen.device_levels = static_cast<uint8_t*>(device_levels);
	for (unsigned int i = 0; i < layout.level_count; i++) gen.texels_offset[i] = layout.texels_offset[i];
	gen.stream = hip_stream;
	return ASTCENC_SUCCESS;
}

/* The options of the _ex_ calls (null: none) into the job, with the constants the host derives from them (mip_post.h). */
static astcenc_error check_mip_options(const char* fn, const astcenc_context* ctx, const astcenc_amd_mip_options* options, MipChainJob& gen)
{
	if (!options || options->flags == 0) return ASTCENC_SUCCESS;
	const unsigned int known = ASTCENC_AMD_MIP_NORMALIZE | ASTCENC_AMD_MIP_ALPHA_COVERAGE;
	if (options->flags & ~known)
	{
		backend_log("%s: options->flags 0x%x has unknown bits 0x%x", fn, options->flags, options->flags & ~known);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const float cutoff = options->alpha_cutoff;
	if ((options->flags & ASTCENC_AMD_MIP_ALPHA_COVERAGE) && !(cutoff > 0.0f && cutoff <= 1.0f))
	{
		backend_log("%s: options->alpha_cutoff %g is not in (0, 1]", fn, (double)cutoff);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (sRGB codes are not the linear components of a vector)
	if ((options->flags & ASTCENC_AMD_MIP_NORMALIZE) && ctx->config.profile == ASTCENC_PRF_LDR_SRGB)
	{
		backend_log("%s: options->flags has ASTCENC_AMD_MIP_NORMALIZE in an ASTCENC_PRF_LDR_SRGB context", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	gen.post_flags = options->flags;
	if (options->flags & ASTCENC_AMD_MIP_ALPHA_COVERAGE)
	{
		gen.alpha_cutoff = cutoff;
		gen.cover_t = mip_cover_u8_threshold(cutoff);
		mip_cover_bounds(cutoff, gen.data_type == ASTCENC_TYPE_F16, gen.cover_hi, gen.cover_lo);
	}
	return ASTCENC_SUCCESS;
}

/* The filter of the _filtered_ calls (null: the box) into the job (its kind and dimensions set): the box leaves it as it is (kind 0,
 * the box kernels). */
static astcenc_error check_mip_filter(const char* fn, const astcenc_amd_mip_filter* filter, MipChainJob& gen)
{
	if (!filter) return ASTCENC_SUCCESS;
	const int kind = (int)filter->kind, edge = (int)filter->edge;
	if (kind < ASTCENC_AMD_MIP_FILTER_BOX || kind > ASTCENC_AMD_MIP_FILTER_KAISER)
	{
		backend_log("%s: filter->kind %d is not an astcenc_amd_mip_filter_kind", fn, kind);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (edge < ASTCENC_AMD_MIP_EDGE_CLAMP || edge > ASTCENC_AMD_MIP_EDGE_CUBE)
	{
		backend_log("%s: filter->edge %d is not an astcenc_amd_mip_edge", fn, edge);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (a cube map: square faces, six layers to a cube; checked for the box too, which never leaves a face)
	if (edge == ASTCENC_AMD_MIP_EDGE_CUBE && (gen.kind != ASTCENC_AMD_MIP_ARRAY || gen.dim_x != gen.dim_y || gen.dim_z % 6u != 0))
	{
		backend_log("%s: filter->edge ASTCENC_AMD_MIP_EDGE_CUBE needs kind ASTCENC_AMD_MIP_ARRAY, dim_x == dim_y and dim_z %% 6 == 0 "
		            "(kind %u, dim_x %u, dim_y %u, dim_z %u)", fn, gen.kind, gen.dim_x, gen.dim_y, gen.dim_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (kind == ASTCENC_AMD_MIP_FILTER_BOX) return ASTCENC_SUCCESS;
	gen.filter_kind = (uint32_t)kind;
	gen.filter_edge = (uint32_t)edge;
	return ASTCENC_SUCCESS;
}

/* The weighting of the _weighted_ calls (null: none) into the job: none leaves it as it is (weight 0, the plain kernels). */
static astcenc_error check_mip_weighting(const char* fn, const astcenc_amd_mip_weighting* weighting, MipChainJob& gen)
{
	if (!weighting) return ASTCENC_SUCCESS;
	const int weight = (int)weighting->weight;
	if (weight != ASTCENC_AMD_MIP_WEIGHT_NONE && weight != ASTCENC_AMD_MIP_WEIGHT_ALPHA)
	{
		backend_log("%s: weighting->weight %d is not an astcenc_amd_mip_weight", fn, weight);
		return ASTCENC_ERR_BAD_PARAM;
	}
	gen.weight = (uint32_t)weight;
	return ASTCENC_SUCCESS;
}

/* The generation and compression entry points; fn: the name of the one called, for the log; options, filter, weighting: null
 * for the calls without them. */
static astcenc_error generate_mip_chain(const char* fn, astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                        unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type, unsigned int level_count,
                                        const astcenc_amd_mip_options* options, const astcenc_amd_mip_filter* filter,
                                        const astcenc_amd_mip_weighting* weighting, void* device_levels, size_t levels_len, void* hip_stream)
{
	if (!ctx) return ASTCENC_ERR_BAD_PARAM;
	struct astcenc_amd_mip_chain_volume_layout layout;
	MipChainJob gen;
	astcenc_error status = check_mip_volume_args(fn, ctx, device_image, dim_x, dim_y, dim_z, kind, data_type, level_count, device_levels, levels_len,
	                                             hip_stream, layout, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_options(fn, ctx, options, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_filter(fn, filter, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_weighting(fn, weighting, gen);
	if (status != ASTCENC_SUCCESS) return status;
	if (layout.level_count == 1) return ASTCENC_SUCCESS;
	status = rc_to_error(backend_generate_mips(ctx->backend, gen));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: device_levels or hip_stream is not on the device of device_image", fn);
	return status;
}

static astcenc_error compress_mip_chain(const char* fn, astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                        unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type, const astcenc_swizzle* swizzle,
                                        unsigned int level_count, const astcenc_amd_mip_options* options, const astcenc_amd_mip_filter* filter,
                                        const astcenc_amd_mip_weighting* weighting, void* device_levels, size_t levels_len,
                                        void* device_blocks, size_t blocks_len, void* hip_stream, float* kernel_ms)
{
	if (!ctx || !swizzle) return ASTCENC_ERR_BAD_PARAM;
	struct astcenc_amd_mip_chain_volume_layout layout;
	MipChainJob gen;
	astcenc_error status = check_mip_volume_args(fn, ctx, device_image, dim_x, dim_y, dim_z, kind, data_type, level_count, device_levels, levels_len,
	                                             hip_stream, layout, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_options(fn, ctx, options, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_filter(fn, filter, gen);
	if (status == ASTCENC_SUCCESS) status = check_mip_weighting(fn, weighting, gen);
	if (status != ASTCENC_SUCCESS) return status;
	if (!device_blocks) { backend_log("%s: device_blocks is null", fn); return ASTCENC_ERR_BAD_CONTEXT; }
	if (blocks_len < layout.blocks_len)
	{
		backend_log("%s: blocks_len %zu, the chain needs %zu", fn, blocks_len, layout.blocks_len);
		return ASTCENC_ERR_OUT_OF_MEM;
	}
	// one set entry per level: level 0 is the caller's image, level i >= 1 lies in device_levels
	std::vector<astcenc_amd_image_set_entry> entries(layout.level_count);
	for (unsigned int i = 0; i < layout.level_count; i++)
	{
		astcenc_amd_image_set_entry& e = entries[i];
		e.image = i == 0 ? const_cast<void*>(device_image) : static_cast<uint8_t*>(device_levels) + layout.texels_offset[i];
		e.blocks = static_cast<uint8_t*>(device_blocks) + layout.blocks_offset[i];
		e.blocks_len = (i + 1 < layout.level_count ? layout.blocks_offset[i + 1] : layout.blocks_len) - layout.blocks_offset[i];
		e.dim_x = layout.dim_x[i]; e.dim_y = layout.dim_y[i]; e.dim_z = layout.dim_z[i];
		e.data_type = data_type;
		e.swizzle = *swizzle;
	}
	status = compress_set(ctx, entries.data(), layout.level_count, hip_stream, kernel_ms, layout.level_count > 1 ? &gen : nullptr);
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: a buffer or hip_stream on another device than device_image, or more than 2^32 - 1 blocks", fn);
	return status;
}

astcenc_error astcenc_amd_generate_mip_chain_volume_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                           unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type,
                                                           unsigned int level_count, void* device_levels, size_t levels_len, void* hip_stream)
{
	return generate_mip_chain("astcenc_amd_generate_mip_chain_volume_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          level_count, nullptr, nullptr, nullptr, device_levels, levels_len, hip_stream);
}

astcenc_error astcenc_amd_compress_mip_chain_volume_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                           unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type,
                                                           const astcenc_swizzle* swizzle, unsigned int level_count, void* device_levels,
                                                           size_t levels_len, void* device_blocks, size_t blocks_len, void* hip_stream,
                                                           float* kernel_ms)
{
	return compress_mip_chain("astcenc_amd_compress_mip_chain_volume_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          swizzle, level_count, nullptr, nullptr, nullptr, device_levels, levels_len, device_blocks, blocks_len, hip_stream, kernel_ms);
}

astcenc_error astcenc_amd_generate_mip_chain_ex_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                       unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type,
                                                       unsigned int level_count, const struct astcenc_amd_mip_options* options,
                                                       void* device_levels, size_t levels_len, void* hip_stream)
{
	return generate_mip_chain("astcenc_amd_generate_mip_chain_ex_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          level_count, options, nullptr, nullptr, device_levels, levels_len, hip_stream);
}

astcenc_error astcenc_amd_compress_mip_chain_ex_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                       unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type,
                                                       const astcenc_swizzle* swizzle, unsigned int level_count,
                                                       const struct astcenc_amd_mip_options* options, void* device_levels, size_t levels_len,
                                                       void* device_blocks, size_t blocks_len, void* hip_stream, float* kernel_ms)
{
	return compress_mip_chain("astcenc_amd_compress_mip_chain_ex_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          swizzle, level_count, options, nullptr, nullptr, device_levels, levels_len, device_blocks, blocks_len, hip_stream, kernel_ms);
}

astcenc_error astcenc_amd_generate_mip_chain_filtered_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x,
                                                             unsigned int dim_y, unsigned int dim_z, astcenc_amd_mip_kind kind,
                                                             astcenc_type data_type, unsigned int level_count,
                                                             const struct astcenc_amd_mip_options* options,
                                                             const struct astcenc_amd_mip_filter* filter, void* device_levels,
                                                             size_t levels_len, void* hip_stream)
{
	return generate_mip_chain("astcenc_amd_generate_mip_chain_filtered_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          level_count, options, filter, nullptr, device_levels, levels_len, hip_stream);
}

astcenc_error astcenc_amd_compress_mip_chain_filtered_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x,
                                                             unsigned int dim_y, unsigned int dim_z, astcenc_amd_mip_kind kind,
                                                             astcenc_type data_type, const astcenc_swizzle* swizzle, unsigned int level_count,
                                                             const struct astcenc_amd_mip_options* options,
                                                             const struct astcenc_amd_mip_filter* filter, void* device_levels,
                                                             size_t levels_len, void* device_blocks, size_t blocks_len, void* hip_stream,
                                                             float* kernel_ms)
{
	return compress_mip_chain("astcenc_amd_compress_mip_chain_filtered_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          swizzle, level_count, options, filter, nullptr, device_levels, levels_len, device_blocks, blocks_len,
	                          hip_stream, kernel_ms);
}

astcenc_error astcenc_amd_generate_mip_chain_weighted_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x,
                                                             unsigned int dim_y, unsigned int dim_z, astcenc_amd_mip_kind kind,
                                                             astcenc_type data_type, unsigned int level_count,
                                                             const struct astcenc_amd_mip_options* options,
                                                             const struct astcenc_amd_mip_filter* filter,
                                                             const struct astcenc_amd_mip_weighting* weighting, void* device_levels,
                                                             size_t levels_len, void* hip_stream)
{
	return generate_mip_chain("astcenc_amd_generate_mip_chain_weighted_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          level_count, options, filter, weighting, device_levels, levels_len, hip_stream);
}

astcenc_error astcenc_amd_compress_mip_chain_weighted_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x,
                                                             unsigned int dim_y, unsigned int dim_z, astcenc_amd_mip_kind kind,
                                                             astcenc_type data_type, const astcenc_swizzle* swizzle, unsigned int level_count,
                                                             const struct astcenc_amd_mip_options* options,
                                                             const struct astcenc_amd_mip_filter* filter,
                                                             const struct astcenc_amd_mip_weighting* weighting, void* device_levels,
                                                             size_t levels_len, void* device_blocks, size_t blocks_len, void* hip_stream,
                                                             float* kernel_ms)
{
	return compress_mip_chain("astcenc_amd_compress_mip_chain_weighted_device", ctx, device_image, dim_x, dim_y, dim_z, kind, data_type,
	                          swizzle, level_count, options, filter, weighting, device_levels, levels_len, device_blocks, blocks_len,
	                          hip_stream, kernel_ms);
}

/* Resizing (mip_resize.h, kernel_resize.hip).  Everything is checked before anything is launched. */
astcenc_error astcenc_amd_resize_image_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                              unsigned int dim_z, astcenc_amd_mip_kind kind, astcenc_type data_type,
                                              const struct astcenc_amd_resize* resize, void* device_out, size_t out_len, void* hip_stream,
                                              float* kernel_ms)
{
	const char* fn = "astcenc_amd_resize_image_device";
	if (!ctx) return ASTCENC_ERR_BAD_PARAM;
	if (!resize) { backend_log("%s: resize is null", fn); return ASTCENC_ERR_BAD_PARAM; }
	if (dim_x == 0 || dim_y == 0 || dim_z == 0 || (int)data_type < ASTCENC_TYPE_U8 || (int)data_type > ASTCENC_TYPE_F32 ||
	    (kind != ASTCENC_AMD_MIP_ARRAY && kind != ASTCENC_AMD_MIP_VOLUME))
	{
		backend_log("%s: dim_x %u, dim_y %u, dim_z %u, kind %d, data_type %d: bad image", fn, dim_x, dim_y, dim_z, (int)kind, (int)data_type);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (resize->dim_x == 0 || resize->dim_y == 0 || resize->dim_z == 0)
	{
		backend_log("%s: resize->dim_x %u, dim_y %u, dim_z %u: a destination dimension is zero", fn, resize->dim_x, resize->dim_y, resize->dim_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const int fkind = (int)resize->filter.kind, edge = (int)resize->filter.edge, weight = (int)resize->weighting.weight;
	if (fkind < ASTCENC_AMD_MIP_FILTER_BOX || fkind > ASTCENC_AMD_MIP_FILTER_KAISER)
	{
		backend_log("%s: resize->filter.kind %d is not an astcenc_amd_mip_filter_kind", fn, fkind);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (edge == ASTCENC_AMD_MIP_EDGE_CUBE)
	{
		backend_log("%s: resize->filter.edge ASTCENC_AMD_MIP_EDGE_CUBE is not supported when resizing", fn);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (edge != ASTCENC_AMD_MIP_EDGE_CLAMP && edge != ASTCENC_AMD_MIP_EDGE_WRAP)
	{
		backend_log("%s: resize->filter.edge %d is not an astcenc_amd_mip_edge", fn, edge);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (weight != ASTCENC_AMD_MIP_WEIGHT_NONE && weight != ASTCENC_AMD_MIP_WEIGHT_ALPHA)
	{
		backend_log("%s: resize->weighting.weight %d is not an astcenc_amd_mip_weight", fn, weight);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (kind == ASTCENC_AMD_MIP_ARRAY && resize->dim_z != dim_z)
	{
		backend_log("%s: resize->dim_z %u changes the %u layers of an ASTCENC_AMD_MIP_ARRAY", fn, resize->dim_z, dim_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const size_t texel_bytes = data_type == ASTCENC_TYPE_U8 ? 4 : data_type == ASTCENC_TYPE_F16 ? 8 : 16;
	bool overflow = false;
	(void)mul_safe(mul_safe(mul_safe(dim_x, dim_y, overflow), dim_z, overflow), texel_bytes, overflow);
	const size_t out_bytes = mul_safe(mul_safe(mul_safe(resize->dim_x, resize->dim_y, overflow), resize->dim_z, overflow), texel_bytes, overflow);
	if (overflow)
	{
		backend_log("%s: the texel bytes of the image or of resize->dim_x %u, dim_y %u, dim_z %u overflow size_t", fn, resize->dim_x,
		            resize->dim_y, resize->dim_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (fkind == ASTCENC_AMD_MIP_FILTER_BOX && data_type == ASTCENC_TYPE_U8)
	{
		// weight x value sums must stay inside 64 bits: den_x den_y den_z 65025 < 2^63
		const unsigned int s[3] = { dim_x, dim_y, kind == ASTCENC_AMD_MIP_VOLUME ? dim_z : 1u };
		const unsigned int d[3] = { resize->dim_x, resize->dim_y, kind == ASTCENC_AMD_MIP_VOLUME ? resize->dim_z : 1u };
		unsigned __int128 den = 65025u;
		for (int a = 0; a < 3; a++)
			if (!mip_resize_passes(s[a], d[a])) den *= s[a] / mip_resize_gcd(s[a], d[a]);
		if (den >= ((unsigned __int128)1 << 63))
		{
			backend_log("%s: resize to %u x %u x %u: the box filter's integer sums would leave 64 bits", fn, resize->dim_x, resize->dim_y,
			            resize->dim_z);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}
	if (!device_image) { backend_log("%s: device_image is null", fn); return ASTCENC_ERR_BAD_CONTEXT; }
	if (!device_out) { backend_log("%s: device_out is null", fn); return ASTCENC_ERR_BAD_CONTEXT; }
	if (out_len < out_bytes)
	{
		backend_log("%s: out_len %zu, resize->dim_x %u, dim_y %u, dim_z %u need %zu", fn, out_len, resize->dim_x, resize->dim_y, resize->dim_z,
		            out_bytes);
		return ASTCENC_ERR_OUT_OF_MEM;
	}
	ResizeJob job;
	memset(&job, 0, sizeof(job));
	job.device_image = device_image; job.device_out = device_out;
	job.dim_x = dim_x; job.dim_y = dim_y; job.dim_z = dim_z;
	job.out_x = resize->dim_x; job.out_y = resize->dim_y; job.out_z = resize->dim_z;
	job.kind = (uint32_t)kind; job.data_type = (uint32_t)data_type;
	job.srgb = ctx->config.profile == ASTCENC_PRF_LDR_SRGB ? 1u : 0u;
	job.filter_kind = (uint32_t)fkind; job.filter_edge = (uint32_t)edge; job.weight = (uint32_t)weight;
	job.stream = hip_stream; job.kernel_ms = kernel_ms;
	const astcenc_error status = rc_to_error(backend_resize(ctx->backend, job));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: device_out or hip_stream is not on the device of device_image", fn);
	if (status == ASTCENC_ERR_OUT_OF_MEM) backend_log("%s: the taps of resize->dim_x %u, dim_y %u, dim_z %u do not fit the scratch bound", fn,
	                                                  resize->dim_x, resize->dim_y, resize->dim_z);
	return status;
}

astcenc_error astcenc_amd_resize_dims(unsigned int dim_x, unsigned int dim_y, unsigned int max_dim, astcenc_amd_resize_pow2 pow2,
                                      unsigned int* out_x, unsigned int* out_y)
{
	if (!out_x || !out_y || (int)pow2 < ASTCENC_AMD_POW2_NONE || (int)pow2 > ASTCENC_AMD_POW2_PREVIOUS) return ASTCENC_ERR_BAD_PARAM;
	unsigned int x, y;
	if (!mip_resize_dims(dim_x, dim_y, max_dim, (unsigned int)pow2, &x, &y)) return ASTCENC_ERR_BAD_PARAM;
	*out_x = x; *out_y = y;
	return ASTCENC_SUCCESS;
}

astcenc_error astcenc_amd_mip_chain_layout(const astcenc_config* config, unsigned int dim_x, unsigned int dim_y, astcenc_type data_type,
                                           unsigned int level_count, struct astcenc_amd_mip_chain_layout* layout)
{
	if (!config || !layout) return ASTCENC_ERR_BAD_PARAM;
	struct astcenc_amd_mip_chain_volume_layout vol;       // (all zero unless it succeeds)
	const astcenc_error status = astcenc_amd_mip_chain_volume_layout(config, dim_x, dim_y, 1, ASTCENC_AMD_MIP_VOLUME, data_type, level_count, &vol);
	memset(layout, 0, sizeof(*layout));
	layout->level_count = vol.level_count;
	memcpy(layout->dim_x, vol.dim_x, sizeof(vol.dim_x));
	memcpy(layout->dim_y, vol.dim_y, sizeof(vol.dim_y));
	memcpy(layout->texels_offset, vol.texels_offset, sizeof(vol.texels_offset));
	memcpy(layout->blocks_offset, vol.blocks_offset, sizeof(vol.blocks_offset));
	layout->texels_len = vol.texels_len;
	layout->blocks_len = vol.blocks_len;
	return status;
}

astcenc_error astcenc_amd_generate_mip_chain_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                    astcenc_type data_type, unsigned int level_count, void* device_levels, size_t levels_len,
                                                    void* hip_stream)
{
	return generate_mip_chain("astcenc_amd_generate_mip_chain_device", ctx, device_image, dim_x, dim_y, 1, ASTCENC_AMD_MIP_VOLUME, data_type,
	                          level_count, nullptr, nullptr, nullptr, device_levels, levels_len, hip_stream);
}

astcenc_error astcenc_amd_compress_mip_chain_device(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y,
                                                    astcenc_type data_type, const astcenc_swizzle* swizzle, unsigned int level_count,
                                                    void* device_levels, size_t levels_len, void* device_blocks, size_t blocks_len,
                                                    void* hip_stream, float* kernel_ms)
{
	return compress_mip_chain("astcenc_amd_compress_mip_chain_device", ctx, device_image, dim_x, dim_y, 1, ASTCENC_AMD_MIP_VOLUME, data_type,
	                          swizzle, level_count, nullptr, nullptr, nullptr, device_levels, levels_len, device_blocks, blocks_len, hip_stream, kernel_ms);
}

} // extern "C"
