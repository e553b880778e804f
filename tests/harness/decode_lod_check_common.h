// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: decode_check_common.h and what the harnesses of the level-of-detail samplers share beyond it
// (decode_lod_check.cpp, decode_lod_grad_check.cpp, decode_cube_check.cpp, decode_volume_check.cpp).  Included after the harness
// has included decode_lod.h or a header on top of it.
#pragma once
#include "decode_check_common.h"

/* The level records of a grid as the kernel finds them: at the record's offset in the table. */
struct LevelsOfGrid {
	const uint8_t* at;
	DecodeLodLevel operator()(uint32_t l) const
	{
		return image_set_record<DecodeLodLevel>(reinterpret_cast<const uint32_t*>(at + (size_t)l * sizeof(DecodeLodLevel)));
	}
};
