// SPDX-License-Identifier: Apache-2.0
// What the host API layer's translation units share: the context and the argument checks of the device-resident entry points.
// astcenc_entry.cpp (linked by the product and by the sequential build of oracle/emu) and astcenc_set.cpp (the image-set entry
// points; product only, since they call backend functions the sequential build does not have).
#pragma once
#include "../../include/astcenc.h"
#include "backend.h"
#include "host_tables.h"

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------------------------
// Context
// ---------------------------------------------------------------------------------------------
struct astcenc_context {
	astcenc_config config;            // validated copy; tune_db_limit already converted
	unsigned int thread_count;
	bool owns_tables;
	const astcenc_context* parent;
	std::vector<uint8_t>* blob;       // table blob (shared with child contexts)
	astcd::HostTables* host_tables;
	astcd::Backend* backend;

	// caller-thread rendezvous for compress (ref: ParallelManager)
	std::mutex lock;
	std::condition_variable cv;
	enum { IDLE, RUNNING, DONE } state;
	astcenc_error result;
	int dstate;                       // same protocol for decompress (ref: manage_decompress)
	astcenc_error dresult;
	std::atomic<int> cancel_flag;     // (ref: ParallelManager::m_is_cancelled, astcenc_internal_entry.h:104)
	int per_slice_fast_load;          // ASTCENC_AMD_OPT_PER_SLICE_FAST_LOAD: -1 not set (each entry point's default), 0, 1
};

struct astcenc_amd_image_set_entry;   // (include/astcenc_amd.h)

namespace astcd {

inline bool swz_ok(astcenc_swz s, bool allow_z)
{
	return (int)s >= ASTCENC_SWZ_R && ((int)s <= ASTCENC_SWZ_1 || (allow_z && s == ASTCENC_SWZ_Z));
}

inline size_t mul_safe(size_t a, size_t b, bool& overflow)
{
	size_t r = a * b;
	overflow = overflow || ((b != 0) && ((r / b) != a));
	return r;
}

inline size_t block_count_axis(size_t dim, size_t block)
{
	size_t n = dim / block;
	if (dim != block * n) n++;
	return n;
}

/* The checks of astcenc_compress_image (ref: Source/astcenc_entry.cpp:1134-1182); block_count: the image's blocks. */
inline astcenc_error check_compress_args(astcenc_context* ctx, unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                         const astcenc_swizzle* swizzle, size_t data_len, unsigned int thread_index, size_t& block_count)
{
	if (ctx->config.flags & ASTCENC_FLG_DECOMPRESS_ONLY) return ASTCENC_ERR_BAD_CONTEXT;
	if (!swz_ok(swizzle->r, false) || !swz_ok(swizzle->g, false) || !swz_ok(swizzle->b, false) || !swz_ok(swizzle->a, false))
	{
		return ASTCENC_ERR_BAD_SWIZZLE;
	}
	if (thread_index >= ctx->thread_count) return ASTCENC_ERR_BAD_PARAM;

	bool overflow = false;
	size_t texel_count = mul_safe(mul_safe(dim_x, dim_y, overflow), dim_z, overflow);
	if (overflow || texel_count == 0) return ASTCENC_ERR_BAD_PARAM;

	size_t bx = block_count_axis(dim_x, ctx->config.block_x);
	size_t by = block_count_axis(dim_y, ctx->config.block_y);
	size_t bz = block_count_axis(dim_z, ctx->config.block_z);
	overflow = false;
	block_count = mul_safe(mul_safe(bx, by, overflow), bz, overflow);
	mul_safe(block_count, 16, overflow);
	if (overflow || block_count == 0) return ASTCENC_ERR_BAD_PARAM;
	if (data_len < block_count * 16) return ASTCENC_ERR_OUT_OF_MEM;
	return ASTCENC_SUCCESS;
}

/* The checks of astcenc_amd_decompress_image_device (those of astcenc_decompress_image, ref: Source/astcenc_entry.cpp:1274-1300,
 * and non-null buffers). */
inline astcenc_error check_decompress_device_args(astcenc_context* ctx, const void* device_blocks, size_t data_len, const void* device_image,
                                                  unsigned int dim_x, unsigned int dim_y, unsigned int dim_z, const astcenc_swizzle* swizzle)
{
	if (!swz_ok(swizzle->r, true) || !swz_ok(swizzle->g, true) || !swz_ok(swizzle->b, true) || !swz_ok(swizzle->a, true))
	{
		return ASTCENC_ERR_BAD_SWIZZLE;
	}
	bool overflow = false;
	size_t texel_count = mul_safe(mul_safe(dim_x, dim_y, overflow), dim_z, overflow);
	if (overflow || texel_count == 0 || !device_blocks || !device_image) return ASTCENC_ERR_BAD_PARAM;
	size_t block_count = mul_safe(mul_safe(block_count_axis(dim_x, ctx->config.block_x), block_count_axis(dim_y, ctx->config.block_y), overflow),
	                              block_count_axis(dim_z, ctx->config.block_z), overflow);
	mul_safe(block_count, 16, overflow);
	if (overflow || block_count == 0) return ASTCENC_ERR_BAD_PARAM;
	if (data_len < block_count * 16) return ASTCENC_ERR_OUT_OF_MEM;
	return ASTCENC_SUCCESS;
}

/* The job of astcenc_amd_compress_volume_device for arguments that check_compress_args has passed: every device-resident
 * compression of one image is this job (astcenc_amd_compress_block_list_device adds its list).
 * A device-resident call is a single-caller operation.  On a thread_count == 1 context it starts from a clean state like
 * astcenc_compress_image does there (a cancel issued before the call is forgotten; one issued while it runs stops it at the
 * next chunk).  On a multi-thread context a cancel is sticky until astcenc_compress_reset -- a device call must not swallow
 * the cancel of a concurrent or later astcenc_compress_image -- so a pending one stops this call as well.  Calls on one
 * context are serialised per device inside the backend. */
inline CompressJob device_compress_job(astcenc_context* ctx, const void* device_image, unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                       astcenc_type data_type, const astcenc_swizzle* swizzle, void* device_out, void* hip_stream, float* kernel_ms)
{
	const bool alpha_scale = ctx->config.a_scale_radius != 0 && ctx->config.block_z <= 1;
	CompressJob job;
	memset(&job, 0, sizeof(job));
	job.device_data = device_image;
	job.dim_x = dim_x;
	job.dim_y = dim_y;
	job.dim_z = dim_z;
	job.data_type = (uint32_t)data_type;
	job.swz[0] = swizzle->r; job.swz[1] = swizzle->g; job.swz[2] = swizzle->b; job.swz[3] = swizzle->a;
	job.device_out = static_cast<uint8_t*>(device_out);
	job.stream = hip_stream;
	job.kernel_ms = kernel_ms;
	job.a_scale_radius = alpha_scale ? ctx->config.a_scale_radius : 0u;
	// default of the device entry points (which have no reference counterpart to match): every slice from its own data
	job.fast_load_slice0 = ctx->per_slice_fast_load == 0 ? 1u : 0u;
	if (ctx->thread_count == 1) ctx->cancel_flag.store(0);
	job.cancel_flag = &ctx->cancel_flag;
	job.progress = ctx->config.progress_callback;
	return job;
}

/* The checks of astcenc_amd_compress_images_device (astcenc_set.cpp) for a set of entry_count >= 1 entries: every entry as
 * astcenc_amd_compress_volume_device checks its image (the log callback names a bad one), and at most 2^32 - 1 blocks in all.
 * jobs[e]: the device-resident fields of entry e's job; total: the blocks of the set. */
astcenc_error check_compress_set(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                 std::vector<CompressJob>& jobs, size_t& total);

} // namespace astcd
