// SPDX-License-Identifier: Apache-2.0
// Windows of compressed images decoded straight into tensors (astcenc_amd_decompress_tensors_device): the work item, the table's
// shape and the lookup are those of decode_regions.h -- a run of at most DECODE_BATCH covered blocks of one block row of one
// region -- and the two compile-time policies of decode_row_batch do the rest.  TensorWindow visits what DecodeWindow visits and
// places a texel at the ELEMENT index of its channel 0 in the region's tensor, mirrored as the region asks; TensorStore takes
// the texel in whichever form it leaves the decoder, makes it the four floats the regions call would have written as the entry's
// data type, and scales, shifts, converts and scatters the first `channels` of them (include/astcenc_amd.h has the arithmetic,
// tests/tensor_model.py spells it out in numpy).
//
// The format holds for a whole call, so its type and layout are template parameters of the sink and the kernel, picked on the host:
// the texel loops hold one kind of store and no dispatch.  `channels`, scale and bias are wave-uniform values of the record.
//
// Included by kernel_decode.hip, tests/harness/decode_tensor_check.cpp and the headers of the other tensor calls (decode_scaled.h,
// decode_sample.h and, through it, decode_lod.h: the format in a record, the texel conversions and TensorStore::put are theirs
// too) only: not part of wave_decode.h's include graph.
//
// Layout: ImageSetTable (count = regions, total = runs), first[count], padding, DecodeTensorRecord[count].  The call's format
// sits in every record rather than in the table's head: a run then reads all it needs with the one block of scalar loads that
// fetches its record (no second address to form, no second wait), and ImageSetTable stays the head every other table has.  It
// costs 48 bytes of upload per region.
#pragma once
#include "decode_regions.h"

namespace astcd { inline namespace ASTC_VARIANT {

/* DecodeWindow's texels, placed in a tensor: `at` is the element index of channel 0, `x_step` elements from column to column
 * (1 planar, `channels` interleaved), rows and slices row / slice elements apart; flags = ASTCENC_AMD_TENSOR_FLIP_*. */
struct TensorWindow {
	DecodeWindow w;                   // (row_texels / slice_texels: the tensor's row and slice pitch in elements)
	uint32_t flags, x_step;
	static constexpr bool whole = false;
	WV_FN int cols_begin(uint32_t x0, int row_len) const { return w.cols_begin(x0, row_len); }
	WV_FN int cols_end(uint32_t x0, int row_len) const { return w.cols_end(x0, row_len); }
	WV_FN int rows_begin(uint32_t y0, int rows) const { return w.rows_begin(y0, rows); }
	WV_FN int rows_end(uint32_t y0, int rows) const { return w.rows_end(y0, rows); }
	WV_FN bool has(uint32_t xi, uint32_t yi, uint32_t zi) const { return w.has(xi, yi, zi); }
	WV_FN size_t at(const DecodeImage&, uint32_t xi, uint32_t yi, uint32_t zi) const
	{
		const uint32_t i = (flags & 1u) ? w.end_x - 1u - xi : xi - w.x;
		const uint32_t j = (flags & 2u) ? w.end_y - 1u - yi : yi - w.y;
		return (size_t)(zi - w.z) * w.slice_texels + (size_t)j * w.row_texels + (size_t)i * x_step;
	}
	// (one image row further down is one tensor row up when mirrored: the sum wraps, as unsigned sums do)
	WV_FN size_t row_step(const DecodeImage&) const { return (flags & 2u) ? (size_t)0 - w.row_texels : w.row_texels; }
};

/* What a run needs of the call's format (wave-uniform, read with its record). */
struct TensorParams {
	uint32_t type, layout, channels, pad;   // (type / layout: the build of the kernel the host launches for this table)
	float    scale[4], bias[4];
	size_t   plane;                   // elements from channel to channel (planar)
};

/* The call's format as a record holds it, `plane_pitch` the region's; ... */
inline TensorParams tensor_params(const DecodeTensorFormat& format, size_t plane_pitch)
{
	TensorParams f;
	memset(&f, 0, sizeof(f));
	f.type = format.type; f.layout = format.layout; f.channels = format.channels;
	// (channels the format does not use are computed and dropped: their factors stay the harmless 0)
	for (uint32_t c = 0; c < format.channels && c < 4u; c++) { f.scale[c] = format.scale[c]; f.bias[c] = format.bias[c]; }
	f.plane = plane_pitch;
	return f;
}

/* ... and the elements from column to column of its tensors: 1 planar, `channels` interleaved. */
inline uint32_t tensor_x_step(const DecodeTensorFormat& format) { return format.layout == 1 ? format.channels : 1u; }

struct DecodeTensorRecord {
	DecodeImage img;                  // the entry's image; data = the region's `out`
	const uint8_t* blocks;
	TensorWindow win;
	TensorParams fmt;
	uint32_t bx0, by0, bz0;           // as DecodeRegionRecord
	uint32_t cols, runs_x, runs_xy;
};
static_assert(sizeof(DecodeTensorRecord) % 8 == 0, "records are read word by word and hold pointers");

/* binary32 -> the bits of a tensor element: round to nearest even, NaNs canonical.  kNumber: y is known not to be a NaN. */
template <bool kNumber> WV_FN uint32_t tensor_f32_bits(float y) { return !kNumber && y != y ? 0x7FC00000u : (uint32_t)float_as_int(y); }
template <bool kNumber> WV_FN uint16_t tensor_f16_bits(float y)
{
	if (!kNumber && y != y) return 0x7E00u;
#if WV_DEVICE
	return __builtin_bit_cast(uint16_t, (_Float16)y);       // v_cvt_f16_f32: nearest even, subnormals produced
#else
	return float_to_half(y);
#endif
}
template <bool kNumber> WV_FN uint16_t tensor_bf16_bits(float y)
{
	if (!kNumber && y != y) return 0x7FC0u;
	const uint32_t u = (uint32_t)float_as_int(y);
	return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);    // (the largest finite values carry into the exponent: infinity)
}

/* binary16 -> binary32, exact (v_cvt_f32_f16 on the device), and the round trip store_texel_at makes for an F16 image. */
WV_FN float tensor_widen_half(uint16_t h)
{
#if WV_DEVICE
	return (float)__builtin_bit_cast(_Float16, h);
#else
	return half_to_float(h);
#endif
}
WV_FN float tensor_through_half(float v)
{
#if WV_DEVICE
	return (float)(_Float16)v;
#else
	return half_to_float(float_to_half(v));
#endif
}

/* A texel in each form it leaves the decoder in, made what the regions call would have stored as the entry's data type
 * (store_texel_at's three routes), as binary32: a packed U8 pixel and four halves as s[0 .. 3]; of an F16 or F32 entry's floats,
 * component c from the swizzle's sources (swizzle_sources; a U8 entry's floats are packed with pack_texel_u8 and go the first
 * way).  Only a pixel's s is known to hold numbers alone.  (tensor_from_source is per component, the loop its callers': with
 * the loop in here the compiler lays one build of astc_decode_tensors out differently.) */
WV_FN void tensor_from_pixel(uint32_t px, float s[4])
{
	s[0] = (float)(px & 0xFFu); s[1] = (float)((px >> 8) & 0xFFu); s[2] = (float)((px >> 16) & 0xFFu); s[3] = (float)(px >> 24);    // v_cvt_f32_ubyte0..3
}
WV_FN void tensor_from_halves(uint64_t px, float s[4])
{
	for (int c = 0; c < 4; c++) s[c] = tensor_widen_half((uint16_t)(px >> (16 * c)));
}
WV_FN float tensor_from_source(const DecodeImage& img, const float src[7], int c)
{
	const float v = src[img.swz[c]];
	return img.data_type == 1 ? tensor_through_half(v) : v;
}

/* The sink: the texel made s[0 .. 3] by the routines above, then one routine.
 * kType / kLayout: astcenc_amd_tensor_type / _layout. */
template <uint32_t kType, uint32_t kLayout>
struct TensorStore {
	TensorParams f;

	template <bool kNumber> static WV_FN uint16_t half_bits(float y) { return kType == 1 ? tensor_f16_bits<kNumber>(y) : tensor_bf16_bits<kNumber>(y); }

	/* y = s[c] * scale[c] + bias[c] as two roundings (the build has -ffp-contract=off), stored as the format's type at element
	 * `at` (+ c planes, or + c).  Planar: lanes hold neighbouring columns, so each channel's store is contiguous across the
	 * wave, in either direction.  Interleaved with four channels: one 8- or 16-byte store.  kNumber: no s[c] is a NaN or an
	 * infinity -- scale and bias are finite, so no y is a NaN and the test for one is left out. */
	template <bool kNumber>
	WV_FN void put(const DecodeImage& img, size_t at, const float s[4]) const
	{
		float y[4];
		for (int c = 0; c < 4; c++) { const float t = s[c] * f.scale[c]; y[c] = t + f.bias[c]; }
		const size_t step = kLayout == 1 ? (size_t)1 : f.plane;
		if (kType == 0)
		{
			float* o = static_cast<float*>(img.data) + at;
			if (kLayout == 1 && f.channels == 4)
			{
				uint32_t v[4];
				for (int c = 0; c < 4; c++) v[c] = tensor_f32_bits<kNumber>(y[c]);
				__builtin_memcpy(o, v, 16);
				return;
			}
			for (int c = 0; c < 4; c++)
				if ((uint32_t)c < f.channels) { const uint32_t v = tensor_f32_bits<kNumber>(y[c]); __builtin_memcpy(o + (size_t)c * step, &v, 4); }
			return;
		}
		uint16_t* o = static_cast<uint16_t*>(img.data) + at;
		if (kLayout == 1 && f.channels == 4)
		{
			uint16_t h[4];
			for (int c = 0; c < 4; c++) h[c] = half_bits<kNumber>(y[c]);
			__builtin_memcpy(o, h, 8);
			return;
		}
		for (int c = 0; c < 4; c++)
			if ((uint32_t)c < f.channels) o[(size_t)c * step] = half_bits<kNumber>(y[c]);
	}

	WV_FN void pixel(const DecodeImage& img, int, size_t at, uint32_t px) const
	{
		float s[4];
		tensor_from_pixel(px, s);
		this->template put<true>(img, at, s);
	}
	WV_FN void halves(const DecodeImage& img, int, size_t at, uint64_t px) const
	{
		float s[4];
		tensor_from_halves(px, s);
		this->template put<false>(img, at, s);
	}
	WV_FN void texel(const DecodeImage& img, int lane, size_t at, float r, float g, float b, float a) const
	{
		if (img.data_type == 0)
		{
			pixel(img, lane, at, pack_texel_u8(img, r, g, b, a));
			return;
		}
		float src[7], s[4];
		swizzle_sources(r, g, b, a, src);
		for (int c = 0; c < 4; c++) s[c] = tensor_from_source(img, src, c);
		this->template put<false>(img, at, s);
	}
	WV_FN void trip_end(int, int, int) const {}
};

inline size_t decode_tensors_bytes(uint32_t count) { return decode_table_bytes<DecodeTensorRecord>(count); }

/* Writes the table of `count` regions over the images `images` (prepared, `data` unused) and their streams; returns the runs
 * of all regions (the caller has made sure they fit 32 bits). */
inline uint32_t decode_tensors_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format,
                                     const DecodeTensorLaunch* regions, uint32_t count)
{
	uint32_t* first;
	DecodeTensorRecord* rec = decode_table_begin<DecodeTensorRecord>(out, decode_tensors_bytes(count), count, first);
	uint32_t runs = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeTensorLaunch& g = regions[i];
		DecodeTensorRecord& r = rec[i];
		r.img = images[g.entry];
		r.img.data = g.d_out;
		r.blocks = streams[g.entry];
		r.win.w.x = g.x; r.win.w.y = g.y; r.win.w.z = g.z;
		r.win.w.end_x = g.x + g.size_x; r.win.w.end_y = g.y + g.size_y; r.win.w.end_z = g.z + g.size_z;
		r.win.w.row_texels = g.row_pitch;
		r.win.w.slice_texels = g.slice_pitch;
		r.win.flags = g.flags;
		r.win.x_step = tensor_x_step(format);
		r.fmt = tensor_params(format, g.plane_pitch);
		uint32_t rows, layers;
		decode_region_cover(g.x, g.size_x, r.img.block_x, r.bx0, r.cols);
		decode_region_cover(g.y, g.size_y, r.img.block_y, r.by0, rows);
		decode_region_cover(g.z, g.size_z, r.img.block_z, r.bz0, layers);
		r.runs_x = (r.cols + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH;
		r.runs_xy = r.runs_x * rows;
		first[i] = runs;
		runs += r.runs_xy * layers;
	}
	return decode_table_finish(out, count, runs);
}

/* Run `local` of the region of `rec` (all 64 lanes call this; `local` is uniform), as decode_region_run; kType / kLayout are
 * the record's. */
template <uint32_t kType, uint32_t kLayout>
WV_FN void decode_tensor_run(const DecodeTensorRecord& rec, uint32_t local, DecodeBatch& batch)
{
	const uint32_t lz = local / rec.runs_xy;
	const uint32_t in_layer = local - lz * rec.runs_xy;
	const uint32_t ly = in_layer / rec.runs_x;
	const uint32_t c0 = (in_layer - ly * rec.runs_x) * (uint32_t)DECODE_BATCH;
	const uint32_t left = rec.cols - c0;
	TensorStore<kType, kLayout> sink = { rec.fmt };
	decode_row_batch(rec.img, rec.blocks, rec.bx0 + c0, rec.by0 + ly, rec.bz0 + lz, (int)(left < (uint32_t)DECODE_BATCH ? left : (uint32_t)DECODE_BATCH), batch, sink, rec.win);
}

} } // namespace astcd::ASTC_VARIANT
