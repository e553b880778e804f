// SPDX-License-Identifier: Apache-2.0
// What the two windowed decoders' entry points share (astcenc_regions.cpp, astcenc_tensors.cpp): the checks of the entries and
// of a window, with the regions call's error codes and log lines.  `fn` names the entry point in the log.
#pragma once
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cstring>
#include <vector>

namespace astcd {

inline astcenc_error windows_rc_to_error(int rc)
{
	return rc == 0 ? ASTCENC_SUCCESS : rc == 1 ? ASTCENC_ERR_OUT_OF_MEM : rc == 3 ? ASTCENC_ERR_BAD_PARAM : ASTCENC_ERR_BAD_CONTEXT;
}

/* Every entry as astcenc_amd_decompress_images_device checks it, `image` aside; jobs[e]: its stream and description. */
inline astcenc_error check_window_entries(const char* fn, astcenc_context* ctx, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                          std::vector<DecompressDeviceJob>& jobs)
{
	jobs.resize(entry_count);
	for (unsigned int e = 0; e < entry_count; e++)
	{
		const astcenc_amd_image_set_entry& en = entries[e];
		// (`image` is not used: the check's non-null test of it sees the stream's pointer)
		astcenc_error status = (int)en.data_type < ASTCENC_TYPE_U8 || (int)en.data_type > ASTCENC_TYPE_F32 ? ASTCENC_ERR_BAD_PARAM :
		                       check_decompress_device_args(ctx, en.blocks, en.blocks_len, en.blocks, en.dim_x, en.dim_y, en.dim_z, &en.swizzle);
		if (status != ASTCENC_SUCCESS)
		{
			backend_log("%s: entry %u of %u: %s", fn, e, entry_count, astcenc_get_error_string(status));
			return status;
		}
		DecompressDeviceJob& job = jobs[e];
		memset(&job, 0, sizeof(job));
		job.device_blocks = static_cast<const uint8_t*>(en.blocks);
		job.dim_x = en.dim_x; job.dim_y = en.dim_y; job.dim_z = en.dim_z;
		job.data_type = (uint32_t)en.data_type;
		job.swz[0] = en.swizzle.r; job.swz[1] = en.swizzle.g; job.swz[2] = en.swizzle.b; job.swz[3] = en.swizzle.a;
	}
	return ASTCENC_SUCCESS;
}

/* Window i of region_count: its entry exists, no size is zero, it lies inside the entry's image. */
inline astcenc_error check_window(const char* fn, unsigned int i, unsigned int region_count, const astcenc_amd_image_set_entry* entries, unsigned int entry_count,
                                  unsigned int entry, unsigned int x, unsigned int y, unsigned int z, unsigned int size_x, unsigned int size_y, unsigned int size_z)
{
	if (entry >= entry_count)
	{
		backend_log("%s: region %u of %u: entry %u, the call has %u entries", fn, i, region_count, entry, entry_count);
		return ASTCENC_ERR_BAD_PARAM;
	}
	const astcenc_amd_image_set_entry& en = entries[entry];
	if (size_x == 0 || size_y == 0 || size_z == 0)
	{
		backend_log("%s: region %u of %u: size %u x %u x %u: a size is zero", fn, i, region_count, size_x, size_y, size_z);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (64 bits: x + size_x may wrap 32)
	if ((unsigned long long)x + size_x > en.dim_x || (unsigned long long)y + size_y > en.dim_y || (unsigned long long)z + size_z > en.dim_z)
	{
		backend_log("%s: region %u of %u: window %u x %u x %u at (%u, %u, %u) is not inside the %u x %u x %u image of entry %u", fn, i, region_count,
		            size_x, size_y, size_z, x, y, z, en.dim_x, en.dim_y, en.dim_z, entry);
		return ASTCENC_ERR_BAD_PARAM;
	}
	return ASTCENC_SUCCESS;
}

/* The running sum of the call's work items after window i; false (logged) past 2^32 - 1. */
inline bool add_window_runs(const char* fn, unsigned int i, unsigned int region_count, const astcenc_context* ctx, const DecodeRegionLaunch& l, unsigned long long& runs)
{
	runs += astc_decode_region_runs(l, ctx->config.block_x, ctx->config.block_y, ctx->config.block_z);
	if (runs <= 0xFFFFFFFFull) return true;
	backend_log("%s: region %u of %u: more than 2^32 - 1 runs of blocks in all", fn, i, region_count);
	return false;
}

} // namespace astcd
