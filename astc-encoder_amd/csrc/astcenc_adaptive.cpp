// SPDX-License-Identifier: Apache-2.0
// Adaptive effort (include/astcenc_amd.h): the block-list launch of the compression kernel, the selection
// of blocks by their error records, and the driver that re-encodes only the blocks that miss a quality target with a stronger
// context and keeps a re-encoded block where it is in fact better; and the same three over an image set -- the levels of a mip
// chain, a batch of textures -- with a block budget (block_budget.h).  Every call checks everything before anything is launched.
// Product library only: the sequential build of oracle/emu has none of the backend functions used here.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cmath>
#include <cstring>
#include <vector>

using namespace astcd;

namespace {

astcenc_error rc_to_error(int rc)
{
	return rc == 0 ? ASTCENC_SUCCESS : rc == 1 ? ASTCENC_ERR_OUT_OF_MEM : rc == 3 ? ASTCENC_ERR_BAD_PARAM : ASTCENC_ERR_BAD_CONTEXT;
}

bool criterion_ok(const astcenc_amd_block_criterion* c)
{
	for (double w : c->channel_weight) if (!std::isfinite(w) || w < 0.0) return false;
	// (a NaN fails the comparison; +inf passes it)
	return c->max_mean_squared_error >= 0.0;
}

} // namespace

extern "C" {

astcenc_error astcenc_amd_compress_block_list_device(astcenc_context* ctx, const void* device_image,
                                                     unsigned int dim_x, unsigned int dim_y, unsigned int dim_z, astcenc_type data_type,
                                                     const astcenc_swizzle* swizzle, const unsigned int* device_list, unsigned int list_count,
                                                     void* device_out, size_t data_len, void* hip_stream, float* kernel_ms)
{
	if (!ctx || !swizzle) return ASTCENC_ERR_BAD_PARAM;
	size_t block_count;
	const astcenc_error status = check_compress_args(ctx, dim_x, dim_y, dim_z, swizzle, data_len, 0, block_count);
	if (status != ASTCENC_SUCCESS) return status;
	// (the list's indices are 32-bit, as the kernel's)
	if (block_count > 0xFFFFFFFFull) return ASTCENC_ERR_BAD_PARAM;
	if (!device_image || !device_out || (!device_list && list_count != 0)) return ASTCENC_ERR_BAD_CONTEXT;
	if (list_count == 0)
	{
		if (kernel_ms) *kernel_ms = 0.0f;
		return ASTCENC_SUCCESS;
	}
	CompressJob job = device_compress_job(ctx, device_image, dim_x, dim_y, dim_z, data_type, swizzle, device_out, hip_stream, kernel_ms);
	job.device_list = device_list;
	job.list_count = list_count;
	return rc_to_error(backend_compress(ctx->backend, job));
}

astcenc_error astcenc_amd_select_blocks_device(astcenc_context* ctx, const astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                               unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                               const astcenc_amd_block_criterion* criterion, unsigned int* device_list, size_t list_len,
                                               void* hip_stream, unsigned int* selected_count)
{
	if (!ctx || !criterion || !selected_count || dim_x == 0 || dim_y == 0 || dim_z == 0 || !criterion_ok(criterion)) return ASTCENC_ERR_BAD_PARAM;
	bool overflow = false;
	const size_t blocks = mul_safe(mul_safe(block_count_axis(dim_x, ctx->config.block_x), block_count_axis(dim_y, ctx->config.block_y), overflow),
	                               block_count_axis(dim_z, ctx->config.block_z), overflow);
	if (overflow || blocks > 0xFFFFFFFFull) return ASTCENC_ERR_BAD_PARAM;
	if (!device_block_errors || !device_list) return ASTCENC_ERR_BAD_CONTEXT;
	if (block_errors_len / sizeof(astcenc_amd_block_error) < blocks || list_len / sizeof(unsigned int) < blocks) return ASTCENC_ERR_OUT_OF_MEM;

	SelectJob job;
	memset(&job, 0, sizeof(job));
	job.device_block_errors = device_block_errors->squared_error;
	job.dim_x = dim_x; job.dim_y = dim_y; job.dim_z = dim_z;
	job.blocks = (uint32_t)blocks;
	for (int i = 0; i < 4; i++) job.weight[i] = criterion->channel_weight[i];
	job.max_mse = criterion->max_mean_squared_error;
	job.device_list = device_list;
	job.stream = hip_stream;
	unsigned int count = 0;
	job.count = &count;
	const int rc = backend_select_blocks(ctx->backend, job);
	if (rc == 0) *selected_count = count;
	return rc_to_error(rc);
}

astcenc_error astcenc_amd_compress_image_adaptive_device(astcenc_context* base, astcenc_context* strong, const void* device_image,
                                                         unsigned int dim_x, unsigned int dim_y, unsigned int dim_z, astcenc_type data_type,
                                                         const astcenc_swizzle* swizzle, const astcenc_swizzle* decode_swizzle,
                                                         const astcenc_amd_block_criterion* criterion, void* device_out, size_t data_len,
                                                         astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                                         void* hip_stream, astcenc_amd_adaptive_stats* stats)
{
	if (!base || !strong || !swizzle || !decode_swizzle || !criterion || !criterion_ok(criterion) || (unsigned)data_type > 2u) return ASTCENC_ERR_BAD_PARAM;
	const astcenc_config& c0 = base->config;
	const astcenc_config& c1 = strong->config;
	if ((c0.flags | c1.flags) & ASTCENC_FLG_DECOMPRESS_ONLY) return ASTCENC_ERR_BAD_CONTEXT;
	if (c0.block_x != c1.block_x || c0.block_y != c1.block_y || c0.block_z != c1.block_z || c0.profile != c1.profile || c0.flags != c1.flags) return ASTCENC_ERR_BAD_PARAM;
	size_t block_count, strong_count;
	astcenc_error status = check_compress_args(base, dim_x, dim_y, dim_z, swizzle, data_len, 0, block_count);
	if (status == ASTCENC_SUCCESS) status = check_compress_args(strong, dim_x, dim_y, dim_z, swizzle, data_len, 0, strong_count);
	if (status != ASTCENC_SUCCESS) return status;
	if (block_count > 0xFFFFFFFFull) return ASTCENC_ERR_BAD_PARAM;
	if (!device_image || !device_out) return ASTCENC_ERR_BAD_CONTEXT;
	status = check_decompress_device_args(strong, device_out, data_len, device_image, dim_x, dim_y, dim_z, decode_swizzle);
	if (status != ASTCENC_SUCCESS) return status;
	if (device_block_errors && block_errors_len / sizeof(astcenc_amd_block_error) < block_count) return ASTCENC_ERR_OUT_OF_MEM;

	// the scratch first, and every buffer on the image's device: without either nothing is written
	int rc = backend_adaptive_reserve(strong->backend, device_image, device_out, device_block_errors, block_count);
	if (rc != 0) return rc_to_error(rc);

	astcenc_amd_adaptive_stats st;
	memset(&st, 0, sizeof(st));
	st.blocks = (unsigned int)block_count;
	CompressJob job = device_compress_job(base, device_image, dim_x, dim_y, dim_z, data_type, swizzle, device_out, hip_stream, stats ? &st.kernel_ms_base : nullptr);
	rc = backend_compress(base->backend, job);
	if (rc != 0) return rc_to_error(rc);
	// (a base pass that was cancelled leaves a partial stream, as astcenc_amd_compress_volume_device does: nothing to refine)
	if (!base->cancel_flag.load())
	{
		AdaptiveJob a;
		memset(&a, 0, sizeof(a));
		a.strong = device_compress_job(strong, device_image, dim_x, dim_y, dim_z, data_type, swizzle, device_out, hip_stream, nullptr);
		a.decode.dim_x = dim_x; a.decode.dim_y = dim_y; a.decode.dim_z = dim_z;
		a.decode.data_type = (uint32_t)data_type;
		a.decode.swz[0] = decode_swizzle->r; a.decode.swz[1] = decode_swizzle->g; a.decode.swz[2] = decode_swizzle->b; a.decode.swz[3] = decode_swizzle->a;
		for (int i = 0; i < 4; i++) a.weight[i] = criterion->channel_weight[i];
		a.max_mse = criterion->max_mean_squared_error;
		a.device_block_errors = device_block_errors ? device_block_errors->squared_error : nullptr;
		a.selected = &st.selected; a.replaced = &st.replaced;
		if (stats) { a.kernel_ms_strong = &st.kernel_ms_strong; a.kernel_ms_other = &st.kernel_ms_other; }
		rc = backend_adaptive_refine(strong->backend, a);
		if (rc != 0) return rc_to_error(rc);
	}
	if (stats) *stats = st;
	return ASTCENC_SUCCESS;
}

/* The image-set forms (include/astcenc_amd.h; the selection: block_budget.h, kernel_select_set.hip). */
astcenc_error astcenc_amd_select_blocks_set_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                   const astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                                   const astcenc_amd_block_criterion* criterion, unsigned int max_blocks,
                                                   unsigned int* device_list, size_t list_len, void* hip_stream,
                                                   unsigned int* candidate_count, unsigned int* selected_count)
{
	const char* fn = "astcenc_amd_select_blocks_set_device";
	if (!ctx || !criterion || !selected_count || !criterion_ok(criterion)) return ASTCENC_ERR_BAD_PARAM;
	if (entry_count == 0)
	{
		if (candidate_count) *candidate_count = 0;
		*selected_count = 0;
		return ASTCENC_SUCCESS;
	}
	if (!entries) { backend_log("%s: entries is null with entry_count %u", fn, entry_count); return ASTCENC_ERR_BAD_PARAM; }
	std::vector<BudgetSetEntry> dims(entry_count);
	size_t blocks = 0;
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		if (en.dim_x == 0 || en.dim_y == 0 || en.dim_z == 0)
		{
			backend_log("%s: image set entry %u of %u: a zero dimension", fn, e, entry_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
		bool overflow = false;
		const size_t n = mul_safe(mul_safe(block_count_axis(en.dim_x, ctx->config.block_x), block_count_axis(en.dim_y, ctx->config.block_y), overflow),
		                          block_count_axis(en.dim_z, ctx->config.block_z), overflow);
		if (overflow || n > 0xFFFFFFFFull || blocks + n > 0xFFFFFFFFull)
		{
			backend_log("%s: image set of %u entries: more than 2^32 - 1 blocks (at entry %u)", fn, entry_count, e);
			return ASTCENC_ERR_BAD_PARAM;
		}
		blocks += n;
		dims[e] = { en.dim_x, en.dim_y, en.dim_z, nullptr };
	}
	if (!device_block_errors || !device_list) return ASTCENC_ERR_BAD_CONTEXT;
	// (the list can never be longer than the budget)
	const size_t list_words = blocks < max_blocks ? blocks : max_blocks;
	if (block_errors_len / sizeof(astcenc_amd_block_error) < blocks || list_len / sizeof(unsigned int) < list_words) return ASTCENC_ERR_OUT_OF_MEM;

	SelectSetJob job;
	memset(&job, 0, sizeof(job));
	job.device_block_errors = device_block_errors->squared_error;
	job.entries = dims.data(); job.count = entry_count; job.blocks = (uint32_t)blocks;
	for (int i = 0; i < 4; i++) job.weight[i] = criterion->channel_weight[i];
	job.max_mse = criterion->max_mean_squared_error;
	job.max_blocks = max_blocks;
	job.device_list = device_list;
	job.stream = hip_stream;
	unsigned int candidates = 0, selected = 0;
	job.candidates = &candidates; job.selected = &selected;
	const int rc = backend_select_blocks_set(ctx->backend, job);
	if (rc == 0)
	{
		if (candidate_count) *candidate_count = candidates;
		*selected_count = selected;
	}
	return rc_to_error(rc);
}

astcenc_error astcenc_amd_compress_block_list_set_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                         const unsigned int* device_list, unsigned int list_count, void* hip_stream, float* kernel_ms)
{
	if (entry_count == 0)
	{
		if (kernel_ms) *kernel_ms = 0.0f;
		return ASTCENC_SUCCESS;
	}
	if (!ctx || !entries) return ASTCENC_ERR_BAD_PARAM;
	std::vector<CompressJob> jobs;
	size_t total;
	const astcenc_error status = check_compress_set(ctx, entries, entry_count, jobs, total);
	if (status != ASTCENC_SUCCESS) return status;
	if (!device_list && list_count != 0) return ASTCENC_ERR_BAD_CONTEXT;
	if (list_count == 0)
	{
		if (kernel_ms) *kernel_ms = 0.0f;
		return ASTCENC_SUCCESS;
	}
	if (ctx->thread_count == 1) ctx->cancel_flag.store(0);
	CompressSetJob set;
	memset(&set, 0, sizeof(set));
	set.entries = jobs.data();
	set.count = entry_count;
	set.stream = hip_stream;
	set.kernel_ms = kernel_ms;
	set.cancel_flag = &ctx->cancel_flag;
	set.progress = ctx->config.progress_callback;
	set.device_list = device_list;
	set.list_count = list_count;
	return rc_to_error(backend_compress_set(ctx->backend, set));
}

astcenc_error astcenc_amd_compress_images_adaptive_device(astcenc_context* base, astcenc_context* strong,
                                                          const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                          const astcenc_swizzle* decode_swizzle, const astcenc_amd_block_criterion* criterion,
                                                          unsigned int max_blocks, astcenc_amd_block_error* device_block_errors,
                                                          size_t block_errors_len, void* hip_stream, astcenc_amd_adaptive_set_stats* stats)
{
	const char* fn = "astcenc_amd_compress_images_adaptive_device";
	if (!base || !strong || !decode_swizzle || !criterion || !criterion_ok(criterion)) return ASTCENC_ERR_BAD_PARAM;
	const astcenc_config& c0 = base->config;
	const astcenc_config& c1 = strong->config;
	if ((c0.flags | c1.flags) & ASTCENC_FLG_DECOMPRESS_ONLY) return ASTCENC_ERR_BAD_CONTEXT;
	if (c0.block_x != c1.block_x || c0.block_y != c1.block_y || c0.block_z != c1.block_z || c0.profile != c1.profile || c0.flags != c1.flags) return ASTCENC_ERR_BAD_PARAM;
	if (entry_count == 0)
	{
		if (stats) memset(stats, 0, sizeof(*stats));
		return ASTCENC_SUCCESS;
	}
	if (!entries) { backend_log("%s: entries is null with entry_count %u", fn, entry_count); return ASTCENC_ERR_BAD_PARAM; }
	for (unsigned int e = 0; e < entry_count; e++)
		if ((unsigned)entries[e].data_type > 2u)
		{
			backend_log("%s: image set entry %u of %u: unknown data_type %d", fn, e, entry_count, (int)entries[e].data_type);
			return ASTCENC_ERR_BAD_PARAM;
		}
	std::vector<CompressJob> base_jobs, strong_jobs;
	size_t block_count, strong_count;
	astcenc_error status = check_compress_set(base, entries, entry_count, base_jobs, block_count);
	if (status == ASTCENC_SUCCESS) status = check_compress_set(strong, entries, entry_count, strong_jobs, strong_count);
	if (status != ASTCENC_SUCCESS) return status;
	std::vector<QualityEntryJob> score(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		status = check_decompress_device_args(strong, en.blocks, en.blocks_len, en.image, en.dim_x, en.dim_y, en.dim_z, decode_swizzle);
		if (status != ASTCENC_SUCCESS)
		{
			backend_log("%s: image set entry %u of %u: %s", fn, e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		QualityEntryJob& q = score[e];
		memset(&q, 0, sizeof(q));
		q.decode.device_blocks = static_cast<const uint8_t*>(en.blocks);
		q.decode.dim_x = en.dim_x; q.decode.dim_y = en.dim_y; q.decode.dim_z = en.dim_z;
		q.decode.data_type = (uint32_t)en.data_type;
		q.decode.swz[0] = decode_swizzle->r; q.decode.swz[1] = decode_swizzle->g; q.decode.swz[2] = decode_swizzle->b; q.decode.swz[3] = decode_swizzle->a;
		q.device_original = en.image; q.original_type = (uint32_t)en.data_type;
	}
	if (device_block_errors && block_errors_len / sizeof(astcenc_amd_block_error) < block_count) return ASTCENC_ERR_OUT_OF_MEM;

	// cancel: the rules of astcenc_amd_compress_images_device, for each context's own pass
	if (base->thread_count == 1) base->cancel_flag.store(0);
	if (strong != base && strong->thread_count == 1) strong->cancel_flag.store(0);
	astcenc_amd_adaptive_set_stats st;
	memset(&st, 0, sizeof(st));
	st.blocks = (unsigned int)block_count;
	CompressSetJob set;
	memset(&set, 0, sizeof(set));
	set.entries = strong_jobs.data();
	set.count = entry_count;
	set.stream = hip_stream;
	set.cancel_flag = &strong->cancel_flag;
	set.progress = strong->config.progress_callback;

	// the scratch first, and every buffer on entry 0's device: without either nothing is written
	int rc = backend_adaptive_set_reserve(strong->backend, set, device_block_errors, block_count);
	if (rc != 0) return rc_to_error(rc);

	CompressSetJob base_set = set;
	base_set.entries = base_jobs.data();
	base_set.kernel_ms = stats ? &st.kernel_ms_base : nullptr;
	base_set.cancel_flag = &base->cancel_flag;
	base_set.progress = base->config.progress_callback;
	rc = backend_compress_set(base->backend, base_set);
	if (rc != 0) return rc_to_error(rc);
	// (a base pass that was cancelled leaves partial streams: nothing to refine)
	if (!base->cancel_flag.load())
	{
		AdaptiveSetJob a;
		memset(&a, 0, sizeof(a));
		a.strong = set;
		a.score = score.data();
		for (int i = 0; i < 4; i++) a.weight[i] = criterion->channel_weight[i];
		a.max_mse = criterion->max_mean_squared_error;
		a.max_blocks = max_blocks;
		a.device_block_errors = device_block_errors ? device_block_errors->squared_error : nullptr;
		a.candidates = &st.candidates; a.selected = &st.selected; a.replaced = &st.replaced;
		if (stats) { a.kernel_ms_strong = &st.kernel_ms_strong; a.kernel_ms_other = &st.kernel_ms_other; }
		rc = backend_adaptive_set_refine(strong->backend, a);
		if (rc != 0) return rc_to_error(rc);
	}
	if (stats) *stats = st;
	return ASTCENC_SUCCESS;
}

} // extern "C"
