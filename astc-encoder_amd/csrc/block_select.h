// SPDX-License-Identifier: Apache-2.0
// The block criterion of astcenc_amd_select_blocks_device and of the adaptive driver (include/astcenc_amd.h,
// struct astcenc_amd_block_criterion): a block's weighted error `e` from its record of four squared-error sums, the number `n` of
// its texels inside the image, and the predicate "selected".  The selection and merge kernels (kernel_select.hip) and the g++
// harness of tests/test_adaptive_cpu.py compile this text.
//
// The units are those of the records (astcenc_amd_compare_blocks_device): U8 as value / 255, floats clamped to 0..65504.  For
// equal RGBA weights a PSNR target of p dB corresponds to max_mean_squared_error = 4 * 10^(-p/10).
//
// No includes and no HIP types.  Every operation of `e` and of the threshold is a separately rounded fp64 operation: the
// library and the harness are compiled with -ffp-contract=off, and the pragma below says so to a compiler that is not.
#pragma once

#if defined(__HIPCC__)
#define ASTC_SELECT_FN __host__ __device__ inline
#else
#define ASTC_SELECT_FN inline
#endif

namespace astcd {

/* e = ((w0 s0 + w1 s1) + w2 s2) + w3 s3, in that order.  (0 * inf is a NaN, which never selects.) */
ASTC_SELECT_FN double block_select_error(const double w[4], double s0, double s1, double s2, double s3)
{
#if defined(__clang__)
	#pragma clang fp contract(off)
#endif
	const double p0 = w[0] * s0, p1 = w[1] * s1, p2 = w[2] * s2, p3 = w[3] * s3;
	const double a = p0 + p1;
	const double b = a + p2;
	return b + p3;
}

/* The texels of raster block `b` that lie inside a dim_x * dim_y * dim_z image: the footprint clipped on every axis (a 2D
 * footprint over slices has block_z == 1 and counts one slice). */
ASTC_SELECT_FN unsigned int block_select_texels(unsigned int b, unsigned int dim_x, unsigned int dim_y, unsigned int dim_z,
                                                unsigned int block_x, unsigned int block_y, unsigned int block_z)
{
	// (dim / block rounded up without the sum that wraps near 2^32)
	const unsigned int blocks_x = dim_x / block_x + (dim_x % block_x != 0u), blocks_y = dim_y / block_y + (dim_y % block_y != 0u);
	const unsigned int row = b / blocks_x, bx = b - row * blocks_x;
	const unsigned int bz = row / blocks_y, by = row - bz * blocks_y;
	const unsigned int left_x = dim_x - bx * block_x, left_y = dim_y - by * block_y, left_z = dim_z - bz * block_z;
	const unsigned int nx = left_x < block_x ? left_x : block_x;
	const unsigned int ny = left_y < block_y ? left_y : block_y;
	const unsigned int nz = left_z < block_z ? left_z : block_z;
	return nx * ny * nz;
}

/* Selected: e > max_mean_squared_error * n, one rounded multiply; false for a NaN e. */
ASTC_SELECT_FN bool block_select_test(double e, double max_mean_squared_error, unsigned int n)
{
	const double limit = max_mean_squared_error * (double)n;
	return e > limit;
}

} // namespace astcd
