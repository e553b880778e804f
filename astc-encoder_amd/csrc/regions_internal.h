// SPDX-License-Identifier: Apache-2.0
// What the entry points of the windowed and the sampled decoders share (astcenc_regions.cpp, astcenc_tensors.cpp,
// astcenc_scaled.cpp and, through sample_internal.h, astcenc_sample.cpp and astcenc_lod.cpp): the checks of the entries and of a
// window, with the regions call's error codes and log lines; for the four calls that write tensors the checks of the format
// and of an output tensor; the end of every call.  `fn` names the entry point in the log.
#pragma once
#include "../../include/astcenc.h"
#include "../../include/astcenc_amd.h"
#include "backend.h"
#include "entry_internal.h"

#include <cmath>
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

/* The tensor format of a call: not null, its type, layout and channels. */
inline astcenc_error check_tensor_format(const char* fn, const astcenc_amd_tensor_format* format)
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

/* ... and its factors, which are finite; fmt: the (checked) format for the backend.  A check of its own: the calls make the
 * checks of their other arguments (a filter, a sampler, the footprint) between the two. */
inline astcenc_error check_tensor_factors(const char* fn, const astcenc_amd_tensor_format* format, DecodeTensorFormat& fmt)
{
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

/* The output tensor of `noun` ("region", "grid") i of count, size_x x size_y elements a channel and size_z slices of them
 * (0: the call's tensors have no slice pitch): the caller's pitches -- in elements, 0 for the tight one -- are at least the
 * tight ones and no product overflows 64 bits, the tensor's extent in bytes among them; the interleaved layout has no plane
 * pitch; `out` is not null and is aligned to an element.  The pitches come back resolved (plane 0 for the interleaved layout).
 * `overflow`: a product of the caller's own has overflowed already; `also_null`: the name of another buffer of the same
 * region that is null, reported where a null `out` is and after it. */
struct TensorPitches { size_t row, slice, plane; };

inline astcenc_error check_output_tensor(const char* fn, const char* noun, unsigned int i, unsigned int count, const astcenc_amd_tensor_format* format,
                                         unsigned int size_x, unsigned int size_y, unsigned int size_z, TensorPitches& p, const void* out,
                                         bool overflow = false, const char* also_null = nullptr, const char* out_name = "out")
{
	const bool planar = format->layout == ASTCENC_AMD_TENSOR_PLANAR;
	const size_t element = format->type == ASTCENC_AMD_TENSOR_F32 ? 4 : 2;
	const size_t tight_row = mul_safe(size_x, planar ? 1 : format->channels, overflow);
	const size_t row_pitch = p.row ? p.row : tight_row;
	const size_t tight_slice = mul_safe(row_pitch, size_y, overflow);
	const size_t slice_pitch = size_z != 0 && p.slice ? p.slice : tight_slice;
	const size_t tight_plane = mul_safe(slice_pitch, size_z != 0 ? size_z : 1, overflow);
	const size_t plane_pitch = p.plane ? p.plane : tight_plane;
	(void)mul_safe(planar ? mul_safe(plane_pitch, format->channels, overflow) : tight_plane, element, overflow);
	if (overflow || row_pitch < tight_row || slice_pitch < tight_slice || (planar && plane_pitch < tight_plane))
	{
		// (the wording is the call's own on purpose: a tensors call's window has a slice pitch, the other calls' outputs have none)
		if (size_z != 0)
			backend_log("%s: %s %u of %u: row_pitch %zu, slice_pitch %zu, plane_pitch %zu: the window needs at least %zu, %zu and %zu elements", fn, noun, i,
			            count, p.row, p.slice, p.plane, tight_row, tight_slice, tight_plane);
		else
			backend_log("%s: %s %u of %u: row_pitch %zu, plane_pitch %zu: the output needs at least %zu and %zu elements", fn, noun, i, count, p.row, p.plane,
			            tight_row, tight_plane);
		return ASTCENC_ERR_BAD_PARAM;
	}
	if (!planar && p.plane != 0)
	{
		backend_log("%s: %s %u of %u: plane_pitch %zu: the interleaved layout has no planes", fn, noun, i, count, p.plane);
		return ASTCENC_ERR_BAD_PARAM;
	}
	// (a null buffer: what the other device calls return for one)
	if (!out || also_null)
	{
		backend_log("%s: %s %u of %u: %s is null", fn, noun, i, count, !out ? out_name : also_null);
		return ASTCENC_ERR_BAD_CONTEXT;
	}
	if (reinterpret_cast<uintptr_t>(out) % element != 0)
	{
		backend_log("%s: %s %u of %u: %s %p is not aligned to the element size %zu", fn, noun, i, count, out_name, out, element);
		return ASTCENC_ERR_BAD_PARAM;
	}
	p.row = row_pitch; p.slice = slice_pitch; p.plane = planar ? plane_pitch : 0;
	return ASTCENC_SUCCESS;
}

/* The end of a call whose arguments are all checked: `job` -- its fields of the call's own filled in by the caller -- gets
 * the entries and the stream and goes to `backend`; the backend's return code as the call's error. */
template <class Job>
inline astcenc_error run_windows_job(const char* fn, astcenc_context* ctx, const std::vector<DecompressDeviceJob>& entries, void* hip_stream, Job& job,
                                     int (*backend)(Backend*, const Job&))
{
	job.entries = entries.data();
	job.entry_count = (uint32_t)entries.size();
	job.stream = hip_stream;
	const astcenc_error status = windows_rc_to_error(backend(ctx->backend, job));
	if (status == ASTCENC_ERR_BAD_PARAM) backend_log("%s: a buffer or hip_stream is not on the device of entry 0's blocks", fn);
	return status;
}

} // namespace astcd
