// SPDX-License-Identifier: Apache-2.0
// The compression kernel's device side: one 64-lane wavefront (= one workgroup) compresses one ASTC block; its working set
// is a dynamic-LDS region laid out by make_lds_layout().  Included by kernel_impl.h (the builds that are part of the library)
// and, as it is, by the translation unit the library writes and compiles at run time for one context (kernel_jit.cpp): no
// host code and no C library header in here or in anything it includes.  The including file sets
//   ASTC_VARIANT     inline-namespace tag of this build of the wave_*.h code
//   ASTC_ENABLE_HDR  0: LDR/sRGB profiles only (HDR endpoint coders compiled out), 1: everything
//   ASTC_KERNEL_NAME
#pragma once
#include "wave_block.h"
#include "image_set.h"
#include "block_tickets.h"

#ifndef ASTC_KERNEL_LINKAGE
#define ASTC_KERNEL_LINKAGE
#endif

#ifndef ASTC_WAVES_PER_EU
#define ASTC_WAVES_PER_EU 4
#endif

namespace astcd {

/* blockIdx -> ASTC block.  Workgroups are dealt round-robin to the 8 XCDs (block b -> XCD b % 8),
 * each with its own L2.  Raster-adjacent ASTC blocks share input cache lines, so every XCD gets a
 * contiguous run of the chunk rather than every 8th block. */
__device__ inline uint32_t xcd_block_remap(uint32_t b, uint32_t n)
{
	const uint32_t per = n / 8u;
	const uint32_t even = per * 8u;
	if (b >= even) return b;               // ragged tail keeps identity order
	return (b % 8u) * per + (b / 8u);
}

/* ... the same for the launches of an image set, in runs of XCD_SET_RUN blocks dealt round-robin: a set mixes images whose
 * blocks cost differently (the levels of a mip chain, textures of several kinds), and with one contiguous eighth per XCD the
 * XCDs that drew the costly entries would run on alone at the end.  A run still keeps raster neighbours together. */
constexpr uint32_t XCD_SET_RUN = 1024;
__device__ inline uint32_t xcd_block_remap_runs(uint32_t b, uint32_t n)
{
	const uint32_t group = XCD_SET_RUN * 8u;
	const uint32_t even = n / group * group;
	if (b >= even) return b;               // ragged tail keeps identity order
	const uint32_t g = b / group, r = b - g * group;
	return g * group + (r % 8u) * XCD_SET_RUN + r / 8u;
}

/* The kernel's arguments as they lie in its argument segment (the declaration below, member for member).  The ticket heads of
 * the launch travel in `img` (astc_tables.h): the argument list is the same for every build, the run-time ones included. */
struct CompressKernelArgs {
	const uint8_t* tab;
	ImageDesc img;
	uint8_t* out;
	uint32_t first_block, num_blocks;
	unsigned long long* prof;
	const ImageSetTable* set;
};

/* One block of a launch: `index` is its launch index -- blockIdx.x in a launch of one workgroup per block, a ticket's index
 * (block_tickets.h) otherwise.  What a block needs of the kernel's arguments it reads from the argument segment itself (scalar
 * loads), so no register of one block reaches the next one.  What a block leaves behind in LDS is dead when the next one starts,
 * exactly as for the workgroup that follows another on a CU (LDS is not cleared between workgroups): load_block writes the
 * whole BlkInfo and the texel rows, search_block resets the best encoding and the trial caches, and a constant-colour block,
 * which skips the search, writes every Scb field its 16 bytes are made from. */
/* ... read from the segment now: scalar loads through a pointer the optimiser cannot see through, so that what is read lives
 * from here to its last use and is not loaded once in front of the ticket loop and carried across every search. */
__attribute__((always_inline)) __device__ inline CompressKernelArgs compress_kernel_args()
{
	uintptr_t args_bits = reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr());
	asm volatile("" : "+s"(args_bits));
	return image_set_record<CompressKernelArgs>((const __attribute__((address_space(4))) uint32_t*)args_bits);
}

__attribute__((always_inline)) __device__ inline void compress_launch_index(uint32_t index)
{
	WV_LANE_SCOPE;
	typedef const __attribute__((address_space(4))) uint8_t* constant_bytes;
	const CompressKernelArgs a = compress_kernel_args();
	ImageDesc img = a.img;
	uint8_t* __restrict__ out = a.out;
	const uint8_t* __restrict__ tab = a.tab;
	unsigned long long* prof = a.prof;
	const ImageSetTable* __restrict__ set = a.set;
	uint32_t b = (set ? xcd_block_remap_runs(index, a.num_blocks) : xcd_block_remap(index, a.num_blocks)) + a.first_block;
	// A block list (astcenc_amd_compress_block_list_device: img.list): `b` is so far a position in the list, the XCD remap
	// included; the block is the one named there, compressed into its own raster slot.  One scalar load through a constant
	// pointer, as for `tab` below.  An index that is no block of the image (a stale list) ends the block before it touches
	// anything.  With a set (astcenc_amd_compress_block_list_set_device) the list names global indices, which then go through the
	// set's lookup below; the by-value record, otherwise unused in a set launch, carries the list and, as blocks_x * 1 * 1, the set's
	// total, so the bound is the same line.
	if (img.list)
	{
		b = reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(reinterpret_cast<uintptr_t>(img.list))[b];
		if (b >= img.blocks_x * img.blocks_y * img.blocks_z) return;
	}
	uint8_t* lds = lds_base();
#if defined(ASTC_TRACE)
	const uint32_t trace_slot = b;
#endif
	// An image set (astcenc_amd_compress_images_device): `b` counts the blocks of all entries back to back.  The entry that
	// holds it is found in the table (image_set.h); its image record and output replace the by-value ones, and `b` becomes
	// the block's index within the entry.  Scalar loads through a constant pointer, as for `tab` below.
	if (set)
	{
		const constant_bytes t = (constant_bytes)reinterpret_cast<uintptr_t>(set);
		const uint32_t count = reinterpret_cast<const __attribute__((address_space(4))) ImageSetTable*>(t)->count;
		const __attribute__((address_space(4))) uint32_t* first =
			reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(t + image_set_first_offset());
		const uint32_t e = image_set_find(first, count, b);
		const ImageSetEntryDesc rec = image_set_record<ImageSetEntryDesc>(reinterpret_cast<const __attribute__((address_space(4))) uint32_t*>(
			t + image_set_records_offset(count) + (size_t)e * sizeof(ImageSetEntryDesc)));
		img = rec.img;
		out = rec.out;
		b -= first[e];
	}
	// raster block order: x fastest, then y, then z (ref: astcenc_entry.cpp:961-966)
	uint32_t row = b / img.blocks_x;
	uint32_t bx = b - row * img.blocks_x;
	uint32_t bz = img.blocks_z > 1 ? row / img.blocks_y : 0u;
	uint32_t by = row - bz * img.blocks_y;

	// one scalar base for the layout, the config and the tables: every field is then a non-negative immediate offset of
	// it (fields of `tab - CTX_LAYOUT_BACK` written as such cost a 64-bit subtraction per field)
	// (through an integer the optimiser cannot see through, and back as a pointer to constant memory -- a generic pointer
	//  would make every table read a flat load)
	uintptr_t base_bits = reinterpret_cast<uintptr_t>(tab) - CTX_LAYOUT_BACK;
	asm volatile("" : "+s"(base_bits));
	const uint8_t* const base = (const uint8_t*)(constant_bytes)base_bits;
	tab = base + CTX_LAYOUT_BACK;
	Ctx c;
	c.tab = tab;
	c.tab_constant = true;
	c.lds = lds;
#if ASTC_FIXED
	// (a fixed-context build: the three records are constants of this translation unit, wave_ctx.h)
	c.root = &kFixedRoot;
	c.cfg = &kFixedConfig;
	c.L = &kFixedLayout;
#else
	c.root = reinterpret_cast<const TableRoot*>(tab);
	c.cfg = reinterpret_cast<const DeviceConfig*>(base + (CTX_LAYOUT_BACK - CTX_CONFIG_BACK));
	c.L = reinterpret_cast<const LdsLayout*>(base);
#endif
	c.T = (int)c.L->texel_count;
#if defined(ASTC_FIXED_OPAQUE_TEXEL_COUNT)
	// (run-time builds for footprints of more than 64 texels, kernel_jit.cpp: the texel count of the lane loops is NOT a
	//  compile-time constant there.  With it, the builds of the 10x8 and 12x12 footprints -- 80 and 144 texels: the last trip of
	//  a texel loop has exactly sixteen lanes -- produce other bytes than the generic build on a quarter of noisy blocks; the
	//  same source with the same constants through g++ (the sequential build, tests/test_emu_fixed.py) does not, and neither does
	//  this build with the count read back through a register.  Not root-caused: DESIGN.md section 3.1.)
	c.T = wv_uniform(wv_opaque(c.T));
#endif
	c.Tp = (c.T + 3) & ~3;
	c.Ts = lds_row_stride(c.Tp);
#if defined(ASTC_TRACE)
	// trace builds: `prof` is the search trace buffer, one slice per block of the image (wave_ctx.h: TRACE_PUT)
	if (prof) prof = reinterpret_cast<unsigned long long*>(reinterpret_cast<uint32_t*>(prof) + (size_t)trace_slot * TRACE_WORDS_PER_BLOCK);
#endif
	c.prof = prof;

	// header for the out-of-line stage functions (ctx_make)
	WV_ONE
	{
		LdsHeader* h = reinterpret_cast<LdsHeader*>(lds);
		h->base = base;
		h->prof = prof;
		c.blk().block_index = b;
	}
	WV_SYNC();

	PROF_SCOPE(c, PS_TOTAL);
	{
		PROF_SCOPE(c, PS_LOAD);
		if (img.alpha_avg && !block_has_visible_alpha(c, img, bx, by)) load_transparent_block(c);
		else DUP_STAGE(c, DUP_LOAD, load_block(c, img, bx, by, bz));
	}
	compress_block(c, out);
}

/* The XCD the wavefront runs on (0 .. 7): where a workgroup starts to draw tickets.  Placement only: any value gives the same bytes. */
__device__ inline uint32_t home_xcd()
{
	uint32_t x;
	asm("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(x));
	return x % TICKET_HEADS;
}

// (the occupancy bound twice: __launch_bounds__ is a macro of the HIP headers, and the run-time compiler of ROCm 7.0 drops its
//  second argument -- 160 VGPRs, three waves per SIMD -- where hipcc and the ROCm 7.2 run-time compiler honour it)
// img.tickets null: one workgroup per block, blockIdx.x is the launch index.  Else the eight zeroed heads of block_tickets.h: the
// grid is smaller than num_blocks and every workgroup compresses blocks until the heads are exhausted.
// (the arguments are read by compress_launch_index and the loop below from the argument segment: CompressKernelArgs)
ASTC_KERNEL_LINKAGE __global__ void __launch_bounds__(64, ASTC_WAVES_PER_EU) __attribute__((amdgpu_waves_per_eu(ASTC_WAVES_PER_EU)))
ASTC_KERNEL_NAME(const uint8_t* __restrict__ tab, ImageDesc img,
                 uint8_t* __restrict__ out, uint32_t first_block, uint32_t num_blocks, unsigned long long* prof,
                 const ImageSetTable* __restrict__ set)
{
	// The ticket loop: heads home, home + 1, ... each until it is exhausted.  Lane 0 draws, with a relaxed device-scope atomic
	// (the heads are shared by every XCD; a ticket orders nothing but itself), and the wave takes its value.  Without tickets
	// the loop makes its one trip with blockIdx.x.  Two scalars live from one trip to the next: `home` and `dry`.
	typedef __attribute__((address_space(1))) uint32_t* global_words;
	const uint32_t home = img.tickets ? home_xcd() : 0u;
	uint32_t dry = 0;
	for (;;)
	{
		const CompressKernelArgs a = compress_kernel_args();
		uint32_t index = blockIdx.x;
		if (a.img.tickets)
		{
			const global_words heads = (global_words)reinterpret_cast<uintptr_t>(a.img.tickets);
			for (;;)
			{
				if (dry == TICKET_HEADS) return;
				const uint32_t x = ticket_head_after(home, dry);
				uint32_t t = 0;
				WV_ONE t = __hip_atomic_fetch_add(heads + ticket_head_word(x), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				t = wv_uniform(t);
				if (t < ticket_head_count(a.num_blocks, x)) { index = ticket_index(t, x); break; }
				dry++;
			}
		}
		compress_launch_index(index);
		if (!compress_kernel_args().img.tickets) return;
		// (the next block's first LDS writes stay behind this block's last LDS reads)
		WV_SYNC();
	}
}

// CompressKernelArgs against the declaration above: the members have the parameters' types in the parameters' order, nothing
// lies between or behind them, and an argument segment lays its arguments out as a C struct lays out its members.
template <class A, class B> struct same_type { static constexpr bool value = false; };
template <class A> struct same_type<A, A> { static constexpr bool value = true; };
static_assert(same_type<decltype(&ASTC_KERNEL_NAME),
                        void (*)(decltype(CompressKernelArgs::tab), decltype(CompressKernelArgs::img), decltype(CompressKernelArgs::out),
                                 decltype(CompressKernelArgs::first_block), decltype(CompressKernelArgs::num_blocks),
                                 decltype(CompressKernelArgs::prof), decltype(CompressKernelArgs::set))>::value,
              "CompressKernelArgs does not mirror the kernel's parameter list");
static_assert(sizeof(ImageDesc) % 8 == 0 && __builtin_offsetof(CompressKernelArgs, tab) == 0 && __builtin_offsetof(CompressKernelArgs, img) == 8 &&
              __builtin_offsetof(CompressKernelArgs, out) == 8 + sizeof(ImageDesc) && __builtin_offsetof(CompressKernelArgs, first_block) == 16 + sizeof(ImageDesc) &&
              __builtin_offsetof(CompressKernelArgs, num_blocks) == 20 + sizeof(ImageDesc) && __builtin_offsetof(CompressKernelArgs, prof) == 24 + sizeof(ImageDesc) &&
              __builtin_offsetof(CompressKernelArgs, set) == 32 + sizeof(ImageDesc) && sizeof(CompressKernelArgs) == 40 + sizeof(ImageDesc),
              "CompressKernelArgs has members, padding or an order that the kernel's argument segment does not");

} // namespace astcd
