// SPDX-License-Identifier: Apache-2.0
// The image-set entry points (include/astcenc_amd.h): many device-resident images through one chain of kernel launches.
// Every entry is checked exactly as the single-image entry point checks its image, all of them before anything is launched;
// the backend then compresses (decompresses) the blocks of all entries as one range (backend_compress_set).
// Product library only: the sequential build of oracle/emu has no backend_*_set.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

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
	const bool alpha_scale = ctx->config.a_scale_radius != 0 && ctx->config.block_z <= 1;
	std::vector<CompressJob> jobs(entry_count);
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
	return rc_to_error(backend_compress_set(ctx->backend, set));
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

} // extern "C"
