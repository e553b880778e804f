// SPDX-License-Identifier: Apache-2.0
// Adaptive effort (include/astcenc_amd.h): the block-list launch of the compression kernel, the selection
// of blocks by their error records, and the driver that re-encodes only the blocks that miss a quality target with a stronger
// context and keeps a re-encoded block where it is in fact better.  Every call checks everything before anything is launched.
// Product library only: the sequential build of oracle/emu has none of the backend functions used here.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cmath>
#include <cstring>

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

} // extern "C"
