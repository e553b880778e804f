// SPDX-License-Identifier: Apache-2.0
// The block quality entry points (include/astcenc_amd.h): compressed blocks scored against their source images in one device
// pass (backend_compare_blocks_set, kernel_quality.hip).  Every call is an image set -- the single-image calls are sets of one
// entry -- and every entry is checked as astcenc_amd_decompress_image_device checks its image, all of them before anything is
// launched.  Product library only: the sequential build of oracle/emu has no backend_compare_blocks_set.
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cstring>
#include <vector>

using namespace astcd;

namespace {

struct QualityEntry {
	const void* blocks; size_t blocks_len;
	const void* image;
	unsigned int dim_x, dim_y, dim_z;
	astcenc_type image_type, decode_type;
	const astcenc_swizzle* swizzle;
};

/* Checks every entry, then runs the set.  block_errors: null, or the records of all entries back to back.  hdr_sums: null, or
 * the HDR sums of entry 0 (single-image calls only). */
astcenc_error compare_set(astcenc_context* ctx, const QualityEntry* entries, unsigned int entry_count, bool name_entries,
                          astcenc_amd_block_error* block_errors, size_t block_errors_len, void* hip_stream,
                          astcenc_amd_error_sums* sums, astcenc_amd_hdr_error_sums* hdr_sums, int fstop_lo, int fstop_hi)
{
	std::vector<QualityEntryJob> jobs(entry_count);
	std::vector<size_t> texels(entry_count);
	size_t total_blocks = 0;
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const QualityEntry& en = entries[e];
		astcenc_error status = en.swizzle ? check_decompress_device_args(ctx, en.blocks, en.blocks_len, en.image, en.dim_x, en.dim_y, en.dim_z, en.swizzle)
		                                  : ASTCENC_ERR_BAD_PARAM;
		if (status == ASTCENC_SUCCESS && ((unsigned)en.image_type > 2u || (unsigned)en.decode_type > 2u)) status = ASTCENC_ERR_BAD_PARAM;
		if (status != ASTCENC_SUCCESS)
		{
			if (name_entries) backend_log("image set entry %u of %u: %s", e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		const size_t blocks = block_count_axis(en.dim_x, ctx->config.block_x) * block_count_axis(en.dim_y, ctx->config.block_y) *
		                      block_count_axis(en.dim_z, ctx->config.block_z);
		texels[e] = (size_t)en.dim_x * en.dim_y * en.dim_z;
		QualityEntryJob& job = jobs[e];
		memset(&job, 0, sizeof(job));
		job.decode.device_blocks = static_cast<const uint8_t*>(en.blocks);
		job.decode.dim_x = en.dim_x; job.decode.dim_y = en.dim_y; job.decode.dim_z = en.dim_z;
		job.decode.data_type = (uint32_t)en.decode_type;
		job.decode.swz[0] = en.swizzle->r; job.decode.swz[1] = en.swizzle->g; job.decode.swz[2] = en.swizzle->b; job.decode.swz[3] = en.swizzle->a;
		job.device_original = en.image;
		job.original_type = (uint32_t)en.image_type;
		job.device_block_errors = block_errors ? block_errors[total_blocks].squared_error : nullptr;
		total_blocks += blocks;
		if (total_blocks > 0xFFFFFFFFull)
		{
			backend_log("image set of %u entries: more than 2^32 - 1 blocks", entry_count);
			return ASTCENC_ERR_BAD_PARAM;
		}
	}
	if (block_errors && block_errors_len / sizeof(astcenc_amd_block_error) < total_blocks)
	{
		backend_log("block errors: %zu bytes for %zu blocks of %zu bytes each", block_errors_len, total_blocks, sizeof(astcenc_amd_block_error));
		return ASTCENC_ERR_OUT_OF_MEM;
	}

	std::vector<double> raw((size_t)entry_count * METRIC_SUMS_HOST);
	QualitySetJob set;
	memset(&set, 0, sizeof(set));
	set.entries = jobs.data();
	set.count = entry_count;
	set.stream = hip_stream;
	set.sums = raw.data();
	set.hdr = hdr_sums ? 1 : 0; set.fstop_lo = fstop_lo; set.fstop_hi = fstop_hi;
	const int rc = backend_compare_blocks_set(ctx->backend, set);
	if (rc != 0) return rc == 1 ? ASTCENC_ERR_OUT_OF_MEM : rc == 3 ? ASTCENC_ERR_BAD_PARAM : ASTCENC_ERR_BAD_CONTEXT;
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const double* r = raw.data() + (size_t)e * METRIC_SUMS_HOST;
		for (int k = 0; k < 4; k++) { sums[e].squared_error[k] = r[k]; sums[e].alpha_scaled_squared_error[k] = r[4 + k]; }
		sums[e].rgb_peak = r[8];
		sums[e].texels = (double)texels[e];
	}
	if (hdr_sums)
	{
		for (int k = 0; k < 4; k++) { hdr_sums->log2_squared_error[k] = raw[10 + k]; hdr_sums->mpsnr_squared_error[k] = raw[14 + k]; }
		hdr_sums->fstop_lo = fstop_lo; hdr_sums->fstop_hi = fstop_hi;
	}
	return ASTCENC_SUCCESS;
}

astcenc_error compare_blocks(astcenc_context* ctx, const void* device_blocks, size_t data_len, const void* device_image,
                             unsigned int dim_x, unsigned int dim_y, unsigned int dim_z, astcenc_type image_type, astcenc_type decode_type,
                             const astcenc_swizzle* swizzle, astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                             void* hip_stream, astcenc_amd_error_sums* sums, astcenc_amd_hdr_error_sums* hdr_sums, int fstop_lo, int fstop_hi)
{
	if (!ctx || !sums) return ASTCENC_ERR_BAD_PARAM;
	// the f-stop becomes a float exponent (ref: mpsnr_operator: "should be in range [-125, 125]")
	if (hdr_sums && (fstop_lo < -125 || fstop_hi > 125 || fstop_hi < fstop_lo)) return ASTCENC_ERR_BAD_PARAM;
	const QualityEntry en = { device_blocks, data_len, device_image, dim_x, dim_y, dim_z, image_type, decode_type, swizzle };
	return compare_set(ctx, &en, 1, false, device_block_errors, block_errors_len, hip_stream, sums, hdr_sums, fstop_lo, fstop_hi);
}

} // namespace

extern "C" {

astcenc_error astcenc_amd_compare_blocks_device(astcenc_context* ctx, const void* device_blocks, size_t data_len, const void* device_image,
                                                unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                                astcenc_type image_type, astcenc_type decode_type, const astcenc_swizzle* swizzle,
                                                astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                                void* hip_stream, astcenc_amd_error_sums* sums)
{
	return compare_blocks(ctx, device_blocks, data_len, device_image, dim_x, dim_y, dim_z, image_type, decode_type, swizzle,
	                      device_block_errors, block_errors_len, hip_stream, sums, nullptr, 0, 0);
}

astcenc_error astcenc_amd_compare_blocks_hdr_device(astcenc_context* ctx, const void* device_blocks, size_t data_len, const void* device_image,
                                                    unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                                    astcenc_type image_type, astcenc_type decode_type, const astcenc_swizzle* swizzle,
                                                    astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                                    int fstop_lo, int fstop_hi, void* hip_stream,
                                                    astcenc_amd_error_sums* sums, astcenc_amd_hdr_error_sums* hdr_sums)
{
	if (!hdr_sums) return ASTCENC_ERR_BAD_PARAM;
	return compare_blocks(ctx, device_blocks, data_len, device_image, dim_x, dim_y, dim_z, image_type, decode_type, swizzle,
	                      device_block_errors, block_errors_len, hip_stream, sums, hdr_sums, fstop_lo, fstop_hi);
}

astcenc_error astcenc_amd_compare_image_set_device(astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                                   astcenc_amd_block_error* device_block_errors, size_t block_errors_len,
                                                   void* hip_stream, astcenc_amd_error_sums* sums)
{
	if (entry_count == 0) return ASTCENC_SUCCESS;
	if (!ctx || !entries || !sums) return ASTCENC_ERR_BAD_PARAM;
	std::vector<QualityEntry> list(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		list[e] = { en.blocks, en.blocks_len, en.image, en.dim_x, en.dim_y, en.dim_z, en.data_type, en.data_type, &en.swizzle };
	}
	return compare_set(ctx, list.data(), entry_count, true, device_block_errors, block_errors_len, hip_stream, sums, nullptr, 0, 0);
}

} // extern "C"
