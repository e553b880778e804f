// SPDX-License-Identifier: Apache-2.0
// HIP backend for gfx950 (MI355X): device-resident tables, staging buffers, and the compression
// kernel launch.  One 64-lane wavefront (one workgroup) compresses one ASTC block; its working
// set is a dynamic-LDS region laid out by make_lds_layout().
//
// Replaces the reference's CPU block loop (compress_image, Source/astcenc_entry.cpp:891-1043):
// instead of threads pulling 16-block tickets from an atomic counter, the block range of a chunk
// is one kernel launch; chunks give the host cancel/progress points.
#include "backend.h"
#include "block_tickets.h"
#include "kernel_jit.h"
#include "mip_resample.h"

#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <sched.h>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

namespace astcd {

/* The host thread that drives a further device of a sharded call (the calling thread drives the first).  Created with
 * the context's slot, parked on a condition variable between calls, joined when the context goes: a call on N devices
 * wakes N - 1 threads instead of creating and joining them (round 5; a 4096^2 image is 26 ms of work per device, a
 * std::thread launch + join some 50-100 us each).  Concurrent calls on one context take turns per worker (`mu`). */
struct SlotWorker {
	std::mutex mu;                    // one task at a time
	std::mutex state_mu;
	std::condition_variable wake, done_cv;
	std::function<void()> task;
	bool has_task = false, done = true, quit = false, bound = false;
	std::thread thread;
	bool started = false;
};

// Everything that lives on one GPU: the table blob, two streams, events and the staging buffers of the
// host-pointer API.  A context owns one slot per device it may run on (see backend_create).
struct DeviceSlot {
	int device = 0;
	uint8_t* d_base = nullptr;    // device allocation: context records, then the table blob
	uint8_t* d_tab = nullptr;     // the blob inside it
	uint8_t* d_dectab = nullptr;  // the decoder's per-footprint tables inside it (after the blob)
	const double* d_srgb = nullptr;   // the sRGB tables of mip chain generation inside it (after the decoder's)
	hipStream_t stream = nullptr;
	hipStream_t copy_stream = nullptr;   // PCIe traffic of the banded host-pointer path
	hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_copy[2] = {}, ev_band = nullptr, ev_done[3] = {}, ev_out[2] = {};
	hipEvent_t ev_gen = nullptr;  // start of a mip chain's generation: its compression's kernel_ms counts from here
	// pinned staging of the banded host-pointer path: two bands of input in flight, the blocks of two bands on their way back
	uint8_t* h_in[2] = {}; size_t h_in_cap = 0;
	uint8_t* h_out[2] = {}; size_t h_out_cap = 0;
	// staging for the host-pointer API
	void* d_image = nullptr; size_t image_cap = 0;
	uint8_t* d_out = nullptr; size_t out_cap = 0;
	float* d_alpha = nullptr; size_t alpha_cap = 0;   // alpha averages of the a_scale_radius pre-pass
	float* d_alpha_scratch = nullptr; size_t alpha_scratch_cap = 0;   // padded tiles of the pre-pass when they outgrow LDS (large radii)
	uint8_t* d_mip_post = nullptr; size_t mip_post_cap = 0;   // counts, histograms and surface states of the mip post-passes
	uint8_t* d_mip_filter = nullptr; size_t mip_filter_cap = 0;   // the taps of a windowed mip filter (kernel_mip_filter.hip)
	std::vector<uint8_t> h_mip_filter;  // ... and their host copy (kept until the next call: the upload is asynchronous)
	uint8_t* d_set = nullptr; size_t set_cap = 0;     // the table of an image set (image_set.h), compression or decompression
	std::vector<uint8_t> h_set;         // ... and its host copy (kept until the next set call: the upload is asynchronous)
	unsigned long long* d_prof = nullptr;   // stage timers (ASTC_PROFILE builds) / search trace (ASTC_TRACE builds)
	size_t trace_cap = 0;         // bytes at d_prof in ASTC_TRACE builds
	double* d_sums = nullptr;     // totals of the image comparison kernel
	double* d_quality = nullptr; size_t quality_cap = 0;   // partial sums of the block quality kernel (kernel_quality.hip), a fixed size
	double* d_quality_sums = nullptr; size_t quality_sums_cap = 0;   // ... and its totals, per entry of the set
	uint32_t* d_select = nullptr; size_t select_cap = 0;   // per-tile counts of the selection kernels, then the merge's counter (kernel_select.hip)
	uint8_t* d_adaptive = nullptr; size_t adaptive_cap = 0;   // the adaptive driver's stream copy, records and list (backend_adaptive_refine)
	// selection with a block budget (kernel_select_set.hip): the keys, the state and histograms, the set's table and its host copy
	unsigned long long* d_keys = nullptr; size_t keys_cap = 0;
	uint8_t* d_budget_fixed = nullptr; size_t budget_fixed_cap = 0;
	uint8_t* d_budget_tab = nullptr; size_t budget_tab_cap = 0;
	std::vector<uint8_t> h_budget_tab;
	hipEvent_t ev_adapt[2] = {};  // around the adaptive driver's work on the strong context (created on first use)
	std::mutex busy;              // one call at a time per slot: the staging buffers and events are shared state
	std::vector<int> local_cpus;  // host CPUs on the device's NUMA node (Linux sysfs); empty: unknown, no binding
	SlotWorker* worker = nullptr; // the slot's parked host thread (slots 1.. of a multi-device context), or null
	// the context's run-time specialised build on this device (kernel_jit.h): loaded once it is ready, then launched
	// instead of the library's own generic build
	hipModule_t jit_module = nullptr;
	hipFunction_t jit_fn = nullptr;
	bool jit_tried = false;
	// block tickets (block_tickets.h): the heads of the launch in flight, the workgroups the device holds of the library's build
	// and of the run-time build (0: not asked yet, RESIDENT_UNKNOWN: the runtime did not say; compress_grid), and the end of the
	// last ticket launch (every ticket launch waits for it: the heads are one buffer)
	uint32_t* d_tickets = nullptr;
	uint32_t resident_lib = 0, resident_jit = 0;
	hipEvent_t ev_tickets = nullptr;
};

struct Backend {
	std::vector<DeviceSlot*> slots;   // the devices host images are sharded over; fixed at backend_create (slot 0 = default device)
	std::vector<DeviceSlot*> extra;   // slots created on first use for device pointers that live on other GPUs; never sharded over
	std::mutex slots_mu;              // guards `extra`
	std::vector<uint8_t> full;        // host copy of [LdsLayout][DeviceConfig][table blob][decoder tables], uploaded to every slot
	size_t dectab_offset;             // of the decoder tables in it
	size_t srgb_offset;               // of the sRGB tables of mip chain generation in it
	DeviceConfig cfg;
	uint32_t lds_bytes;
	bool hdr;
	TableRoot root;
	int variant;                      // index into kernel_variants (chosen by the first kernel_prepare)
	JitKernel* jit;                   // the context's run-time build (null: none asked for -- a fixed-context build of the library
	                                  // serves this context, ASTCENC_AMD_JIT=off, an instrumentation build, no hipRTC)
	JitMode jit_mode;
	std::atomic<unsigned long long> blocks_done;     // blocks this context has compressed (JIT_LAZY's trigger)
	unsigned long long jit_lazy_blocks;              // ... and the count at which the compile is queued (JIT_LAZY_BLOCKS)
	std::atomic<bool> jit_active;     // some slot launches the run-time build
};

// The library's own device buffers end in a little slack, so that a buffer never stops exactly at the end
// of a mapped page.
constexpr size_t ALLOC_SLACK = 4096;
/* Smallest host image whose PCIe transfers are pipelined against its kernels in bands (compress_on_slot_locked).  A band
 * costs about half a millisecond of its own (a block takes 0.8 ms from load to store, so every kernel ends in a tail that does
 * not fill the device); four bands pay for themselves once the image's transfers take longer than that: measured break-even
 * near 4096 x 4096 at 6x6 (profiles/r06z/host_api_small_images.txt). */
constexpr size_t BAND_MIN_BLOCKS = (size_t)1 << 18;
#if defined(ASTC_TRACE)
constexpr size_t TRACE_WORDS_PER_BLOCK_HOST = 1024;   // = TRACE_WORDS_PER_BLOCK (wave_ctx.h)
#endif

/* Diagnostics.  The library reports through return codes only; what it has to say beyond them -- which HIP call failed,
 * why a device was skipped -- goes to a callback the host application may install (astcenc_amd_set_log_callback,
 * include/astcenc_amd.h), or to stderr when ASTCENC_AMD_LOG=stderr is in the environment.  Nothing is printed otherwise. */
static std::atomic<void (*)(const char*)> g_log_callback{nullptr};
void backend_set_log_callback(void (*cb)(const char*)) { g_log_callback.store(cb); }
static void log_msg(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static void log_msg(const char* fmt, ...)
{
	void (*cb)(const char*) = g_log_callback.load();
	static const bool to_stderr = []() { const char* e = getenv("ASTCENC_AMD_LOG"); return e && strcmp(e, "stderr") == 0; }();
	if (!cb && !to_stderr) return;
	char line[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(line, sizeof(line), fmt, ap);
	va_end(ap);
	if (cb) cb(line);
	else fprintf(stderr, "astcenc_amd: %s\n", line);
}

void backend_log(const char* fmt, ...)
{
	char line[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(line, sizeof(line), fmt, ap);
	va_end(ap);
	log_msg("%s", line);
}

#define HIP_TRY(expr, fail) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	log_msg("%s -> %s", #expr, hipGetErrorString(e_)); fail; } } while (0)

const char* backend_name() { return "hip:gfx950"; }

namespace {

/* The calling thread's current device is the caller's business (a torch process, an engine): every
 * entry point puts it back on exit. */
struct DeviceGuard {
	int saved; bool ok;
	DeviceGuard() : saved(0), ok(hipGetDevice(&saved) == hipSuccess) {}
	~DeviceGuard() { if (ok) (void)hipSetDevice(saved); }
};

/* Grows a staging buffer of the slot to at least `need` bytes (its contents are not kept).  0 ok, 1 out of memory: the buffer is
 * then null and its capacity 0, so that the next call tries again. */
template <class T> int grow(T*& buf, size_t& cap, size_t need)
{
	if (cap >= need) return 0;
	if (buf) (void)hipFree(buf);
	buf = nullptr; cap = 0;
	HIP_TRY(hipMalloc(reinterpret_cast<void**>(&buf), need + ALLOC_SLACK), return 1);
	cap = need;
	return 0;
}
/* ... and a pair of pinned host buffers. */
int grow_pinned(uint8_t* (&pair)[2], size_t& cap, size_t need)
{
	if (cap >= need) return 0;
	for (uint8_t*& h : pair) { if (h) (void)hipHostFree(h); h = nullptr; }
	cap = 0;
	for (uint8_t*& h : pair) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&h), need, hipHostMallocDefault), return 1);
	cap = need;
	return 0;
}

/* The builds of the compression kernel.  Generic ones: LDR / HDR coders x footprints of at most 64 texels (whose texel
 * loops make one trip, kernel_ldr64.hip) / the larger ones.  Fixed-context ones (kernel_ldr_6x6m.hip, ...): compiled for
 * one named context each, its LDS layout, configuration and table root as constants; their `prepare` returns
 * ASTC_PREPARE_NOT_THIS_CONTEXT unless the live context is that one, record for record.  The first variant that accepts
 * the context is used (fixed ones first); ASTCENC_AMD_KERNEL=generic in the environment skips the fixed ones. */
struct KernelVariant {
	const char* name;
	bool fixed, hdr, small;
	int (*prepare)(const TableRoot&, const DeviceConfig&, uint32_t*, void*, uint32_t*);
	int (*launch)(const KernelLaunch&);
	int (*occupancy)(uint32_t, int*);
};
const KernelVariant kernel_variants[] = {
	{ "astc_compress_blocks_ldr_6x6m", true, false, true, astc_kernel_prepare_ldr_6x6m, astc_kernel_launch_ldr_6x6m, astc_kernel_occupancy_ldr_6x6m },
	{ "astc_compress_blocks_ldr_8x8t", true, false, true, astc_kernel_prepare_ldr_8x8t, astc_kernel_launch_ldr_8x8t, astc_kernel_occupancy_ldr_8x8t },
	{ "astc_compress_blocks_hdr_6x6m", true, true, true, astc_kernel_prepare_hdr_6x6m, astc_kernel_launch_hdr_6x6m, astc_kernel_occupancy_hdr_6x6m },
	{ "astc_compress_blocks_ldr64", false, false, true, astc_kernel_prepare_ldr64, astc_kernel_launch_ldr64, astc_kernel_occupancy_ldr64 },
	{ "astc_compress_blocks_hdr64", false, true, true, astc_kernel_prepare_hdr64, astc_kernel_launch_hdr64, astc_kernel_occupancy_hdr64 },
	{ "astc_compress_blocks_ldr", false, false, false, astc_kernel_prepare_ldr, astc_kernel_launch_ldr, astc_kernel_occupancy_ldr },
	{ "astc_compress_blocks_hdr", false, true, false, astc_kernel_prepare_hdr, astc_kernel_launch_hdr, astc_kernel_occupancy_hdr },
};
/* Picks the context's variant (b->variant < 0: not chosen yet) and prepares it on the current device. */
int kernel_prepare(Backend* b, uint32_t* lds_bytes, void* layout_out, uint32_t* layout_bytes)
{
	if (b->variant >= 0) return kernel_variants[b->variant].prepare(b->root, b->cfg, lds_bytes, layout_out, layout_bytes);
	const bool small = b->root.texel_count <= 64;
	const char* want = getenv("ASTCENC_AMD_KERNEL");
	const bool generic_only = want && strcmp(want, "generic") == 0;
	for (int i = 0; i < (int)(sizeof(kernel_variants) / sizeof(kernel_variants[0])); i++)
	{
		const KernelVariant& v = kernel_variants[i];
		if (v.hdr != b->hdr || v.small != small || (v.fixed && generic_only)) continue;
		const int rc = v.prepare(b->root, b->cfg, lds_bytes, layout_out, layout_bytes);
		if (rc == ASTC_PREPARE_NOT_THIS_CONTEXT) continue;
		if (rc == 0) b->variant = i;
		return rc;
	}
	return (int)hipErrorInvalidDeviceFunction;
}
int kernel_launch(const Backend* b, const DeviceSlot* s, const KernelLaunch& k)
{
	if (s->jit_fn)
	{
		// the run-time build: same parameters as the library's builds (kernel_device.h), launched through the module API
		KernelLaunch a = k;
		void* args[] = { &a.d_tab, &a.img, &a.d_out, &a.first, &a.count, &a.d_prof, &a.d_set };
		return (int)hipModuleLaunchKernel(s->jit_fn, k.img.tickets ? k.grid : k.count, 1, 1, 64, 1, 1, k.lds_bytes, static_cast<hipStream_t>(k.stream), args, nullptr);
	}
	return kernel_variants[b->variant].launch(k);
}

/* ASTCENC_AMD_COMPRESS_GRID, read once per process: unset (-1) a launch of more blocks than the device holds workgroups draws
 * its blocks from tickets (block_tickets.h); 0 never; N > 0 every launch does, with min(N, blocks) workgroups (the tests'
 * handle on the ticket path: tests/test_persistent_grid.py). */
long compress_grid_from_env()
{
	static const long v = []() {
		const char* e = getenv("ASTCENC_AMD_COMPRESS_GRID");
		if (!e || !*e) return -1L;
		char* end = nullptr;
		const long n = strtol(e, &end, 10);
		return end != e && n >= 0 && n <= 0x7fffffffL ? n : -1L;
	}();
	return v;
}

/* The workgroups of the build the slot launches that its device holds at once: CUs x workgroups per CU at the context's LDS
 * size, asked once per build (current device = the slot's) and reported once to the diagnostics callback.  0: the runtime
 * does not say; launches then stay one workgroup per block. */
constexpr uint32_t RESIDENT_UNKNOWN = 0xFFFFFFFFu;
uint32_t compress_grid(const Backend* b, DeviceSlot* s)
{
	uint32_t& resident = s->jit_fn ? s->resident_jit : s->resident_lib;
	if (resident) return resident == RESIDENT_UNKNOWN ? 0 : resident;
	int cus = 0, per_cu = 0;
	hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
	if (e == hipSuccess)
		e = s->jit_fn ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, s->jit_fn, 64, b->lds_bytes)
		              : (hipError_t)kernel_variants[b->variant].occupancy(b->lds_bytes, &per_cu);
	if (e != hipSuccess || cus <= 0 || per_cu <= 0)
	{
		(void)hipGetLastError();
		log_msg("occupancy of %s on device %d unknown: one workgroup per block", s->jit_fn ? "the run-time build" : kernel_variants[b->variant].name, s->device);
		resident = RESIDENT_UNKNOWN;
		return 0;
	}
	resident = (uint32_t)cus * (uint32_t)per_cu;
	log_msg("%s on device %d: %u workgroups resident (%d CUs x %d); a launch of more blocks draws them from tickets",
	        s->jit_fn ? "the run-time build" : kernel_variants[b->variant].name, s->device, resident, cus, per_cu);
	return resident;
}

/* Turns `k` into a ticket launch of `grid` workgroups: the heads are zeroed on the launch's stream in front of it.  The slot
 * has one ticket buffer, so the launch first waits for the end of the last ticket launch, whichever stream that was on (no
 * wait at all on the same stream, or before the event was ever recorded). */
int tickets_arm(DeviceSlot* s, KernelLaunch& k, uint32_t grid)
{
	const hipStream_t stream = static_cast<hipStream_t>(k.stream);
	HIP_TRY(hipStreamWaitEvent(stream, s->ev_tickets, 0), return 2);
	HIP_TRY(hipMemsetAsync(s->d_tickets, 0, TICKET_BUFFER_BYTES, stream), return 2);
	k.img.tickets = s->d_tickets;
	k.grid = grid;
	return 0;
}
int tickets_launched(DeviceSlot* s, const KernelLaunch& k)
{
	const hipStream_t stream = static_cast<hipStream_t>(k.stream);
	HIP_TRY(hipEventRecord(s->ev_tickets, stream), return 2);
	return 0;
}

/* The self-check of slot_adopt_jit: 48 x 48 blocks (volumes: 16 x 16 x 8) of deterministic RGBA8 content through `fn` and
 * through the library's build of the context; true when the two block streams are byte-identical.  (2304 blocks, nine content
 * classes: a build compiled with floating-point contraction differs from the generic build on one block in a hundred of
 * grey content and one in four hundred of lightly noisy ramps, and passed the 256 blocks of six classes this check once was
 * -- tests/test_jit_matrix.py keeps such builds and expects them to be turned away here.) */
constexpr uint32_t JIT_SELF_CHECK_GRID = 288;
bool jit_self_check(Backend* b, DeviceSlot* s, hipFunction_t fn)
{
	const uint32_t bsx = b->root.dim_x, bsy = b->root.dim_y, bsz = b->root.dim_z;
	const uint32_t nbx = bsz > 1 ? 16u : 48u, nby = bsz > 1 ? 16u : 48u, nbz = bsz > 1 ? 8u : 1u;
	const uint32_t dim_x = nbx * bsx - 1u, dim_y = nby * bsy - 1u, dim_z = bsz > 1 ? nbz * bsz - 1u : 1u;      // (the last blocks are partial)
	const size_t texels = (size_t)dim_x * dim_y * dim_z, nblocks = (size_t)nbx * nby * nbz;
	std::vector<uint8_t> img(texels * 4);
	uint32_t rng = 0x9E3779B1u;
	auto tri = [](uint32_t v) { const uint32_t m = v & 511u; return (int)(m < 256u ? m : 511u - m); };
	for (uint32_t z = 0; z < dim_z; z++)
		for (uint32_t y = 0; y < dim_y; y++)
			for (uint32_t x = 0; x < dim_x; x++)
			{
				// per block-sized tile: noise amplitude 0 (ramps), 6, 40, 255 (pure noise), two colours, a constant, grey with
				// noise (opaque / with a varying alpha), smooth ramps without a step
				const uint32_t tile = (x / bsx + 3u * (y / bsy) + 5u * (z / bsz) + y / (3u * bsy)) % 9u;
				uint8_t* px = &img[(((size_t)z * dim_y + y) * dim_x + x) * 4];
				int grey = 0;
				for (int ch = 0; ch < 4; ch++)
				{
					rng = rng * 1664525u + 1013904223u;
					const int noise = (int)(rng >> 24);
					int v = (int)((x * (3u + ch) + y * (7u - ch) + z * 11u) & 255u);
					if (tile == 1) v += (noise & 15) - 6;
					else if (tile == 2) v += (noise & 63) - 24;
					else if (tile == 3) v = noise;
					else if (tile == 4) v = ((x + ch) ^ (y >> 1)) & 2 ? 220 - 20 * ch : 30 + 25 * ch;
					else if (tile == 5) v = 40 + 50 * ch;
					else if (tile == 6 || tile == 7)
					{
						if (ch == 0) grey = (3 * tri(x + 2u * y + 5u * z) + tri((3u * x + 512u - y) >> 1)) / 4 + noise % 21 - 10;
						v = ch < 3 ? grey : 192 + tri((x >> 1) + (y >> 2)) / 4 + noise % 7 - 3;
					}
					else if (tile == 8) v = tri(x * (2u + ch) + y * (5u - ch) + z * 3u);
					if (ch == 3 && tile != 3 && tile != 2 && tile != 7) v = 255;
					px[ch] = (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
				}
			}
	void* d_img = nullptr;
	uint8_t* d_out = nullptr;
	bool ok = hipMalloc(&d_img, img.size() + ALLOC_SLACK) == hipSuccess && hipMalloc(reinterpret_cast<void**>(&d_out), 2 * nblocks * 16 + ALLOC_SLACK) == hipSuccess;
	std::vector<uint8_t> out(2 * nblocks * 16);
	if (ok)
	{
		CompressJob job;
		memset(&job, 0, sizeof(job));
		job.dim_x = dim_x; job.dim_y = dim_y; job.dim_z = dim_z;
		for (int i = 0; i < 4; i++) job.swz[i] = (uint32_t)i;
		KernelLaunch k;
		k.d_tab = s->d_tab; k.lds_bytes = b->lds_bytes; k.d_prof = nullptr; k.d_set = nullptr; k.stream = s->stream;
		k.first = 0; k.count = (uint32_t)nblocks;
		k.img = image_desc(b->root, b->cfg.profile, job, d_img);
		ok = hipMemcpyAsync(d_img, img.data(), img.size(), hipMemcpyHostToDevice, s->stream) == hipSuccess;
		k.d_out = d_out;
		ok = ok && kernel_variants[b->variant].launch(k) == 0;
		k.d_out = d_out + nblocks * 16;
		// (the candidate through the ticket path, 288 workgroups over the 2304 blocks: every workgroup compresses several blocks of
		//  different classes one after the other, so a build that carries state from one block into the next is turned away too)
		ok = ok && tickets_arm(s, k, JIT_SELF_CHECK_GRID) == 0;
		void* args[] = { &k.d_tab, &k.img, &k.d_out, &k.first, &k.count, &k.d_prof, &k.d_set };
		ok = ok && hipModuleLaunchKernel(fn, k.grid, 1, 1, 64, 1, 1, k.lds_bytes, s->stream, args, nullptr) == hipSuccess;
		ok = ok && tickets_launched(s, k) == 0;
		ok = ok && hipMemcpyAsync(out.data(), d_out, out.size(), hipMemcpyDeviceToHost, s->stream) == hipSuccess;
		ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
		if (!ok) (void)hipGetLastError();
	}
	if (d_img) (void)hipFree(d_img);
	if (d_out) (void)hipFree(d_out);
	return ok && memcmp(out.data(), out.data() + nblocks * 16, nblocks * 16) == 0;
}

/* Loads the context's run-time build on the slot's device once the compiler has delivered it (current device = the slot's).
 * Anything that goes wrong leaves the slot on the library's generic build. */
void slot_adopt_jit(Backend* b, DeviceSlot* s)
{
	if (!b->jit || s->jit_tried || jit_state(b->jit) != JIT_READY) return;
	s->jit_tried = true;
	size_t bytes = 0;
	const void* code = jit_code(b->jit, &bytes);
	hipModule_t mod = nullptr;
	hipFunction_t fn = nullptr;
	if (hipModuleLoadData(&mod, code) != hipSuccess || hipModuleGetFunction(&fn, mod, JIT_ENTRY_POINT) != hipSuccess)
	{
		(void)hipGetLastError();
		if (mod) (void)hipModuleUnload(mod);
		log_msg("run-time build %s does not load on device %d: the generic build stays", jit_kernel_name(b->jit), s->device);
		return;
	}
	// Trust, but verify: before the build takes over, it and the library's own build compress the same 2304 blocks of built-in
	// content -- noise of several amplitudes over ramps, flat, two-colour, grey and smooth stretches, i.e. blocks that run every
	// trial of the search -- and the bytes must be equal.  (A build is compiled from the same source with the same numerics flags, so they
	// are -- unless the compiler did something with the constants that it does not do without them: the run-time builds of the
	// 10x8 and 12x12 footprints do differ, DESIGN.md section 3.1, and are turned away here.)
	// (ASTCENC_AMD_JIT_SELF_CHECK=0: debugging only -- tools/jit_debug4.py looks at a build the check turns away)
	const char* check = getenv("ASTCENC_AMD_JIT_SELF_CHECK");
	if (!(check && strcmp(check, "0") == 0) && !jit_self_check(b, s, fn))
	{
		(void)hipModuleUnload(mod);
		log_msg("run-time build %s does not reproduce the generic build's bytes on the self-check image: the generic build stays", jit_kernel_name(b->jit));
		return;
	}
	s->jit_module = mod;
	s->jit_fn = fn;
	b->jit_active.store(true);
}

void worker_stop(SlotWorker* w)
{
	if (!w) return;
	if (w->started)
	{
		{ std::lock_guard<std::mutex> g(w->state_mu); w->quit = true; }
		w->wake.notify_one();
		w->thread.join();
	}
	delete w;
}

void slot_destroy(DeviceSlot* s)
{
	if (!s) return;
	worker_stop(s->worker);
	s->worker = nullptr;
	(void)hipSetDevice(s->device);
	if (s->d_image) (void)hipFree(s->d_image);
	if (s->d_out) (void)hipFree(s->d_out);
	if (s->d_alpha) (void)hipFree(s->d_alpha);
	if (s->d_alpha_scratch) (void)hipFree(s->d_alpha_scratch);
	if (s->d_mip_post) (void)hipFree(s->d_mip_post);
	if (s->d_mip_filter) (void)hipFree(s->d_mip_filter);
	if (s->d_set) (void)hipFree(s->d_set);
	if (s->d_sums) (void)hipFree(s->d_sums);
	if (s->d_quality) (void)hipFree(s->d_quality);
	if (s->d_quality_sums) (void)hipFree(s->d_quality_sums);
	if (s->d_select) (void)hipFree(s->d_select);
	if (s->d_adaptive) (void)hipFree(s->d_adaptive);
	if (s->d_keys) (void)hipFree(s->d_keys);
	if (s->d_budget_fixed) (void)hipFree(s->d_budget_fixed);
	if (s->d_budget_tab) (void)hipFree(s->d_budget_tab);
	for (hipEvent_t e : s->ev_adapt) if (e) (void)hipEventDestroy(e);
	if (s->d_prof) (void)hipFree(s->d_prof);
	if (s->d_tickets) (void)hipFree(s->d_tickets);
	if (s->ev_tickets) (void)hipEventDestroy(s->ev_tickets);
	for (int i = 0; i < 2; i++) { if (s->h_in[i]) (void)hipHostFree(s->h_in[i]); if (s->h_out[i]) (void)hipHostFree(s->h_out[i]); }
	for (hipEvent_t e : { s->ev_copy[0], s->ev_copy[1], s->ev_band, s->ev_done[0], s->ev_done[1], s->ev_done[2], s->ev_out[0], s->ev_out[1], s->ev0, s->ev1, s->ev_gen })
		if (e) (void)hipEventDestroy(e);
	if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
	if (s->stream) (void)hipStreamDestroy(s->stream);
	if (s->jit_module) (void)hipModuleUnload(s->jit_module);
	if (s->d_base) (void)hipFree(s->d_base);
	delete s;
}

/* The host CPUs next to `device` (Linux: /sys/bus/pci/devices/<bus id>/local_cpulist, e.g. "0-31,128-159").  A shard's
 * worker thread runs on them (bind_worker_to_device), so the pinned staging buffers it allocates on first use -- pinned
 * pages are placed by first touch -- and the memcpy into them stay on the device's NUMA node: on an 8-GPU node the
 * other placement sends every band across the inter-socket link twice.  Empty when the platform does not say. */
static std::vector<int> device_local_cpus(int device)
{
	std::vector<int> cpus;
	char bus[64] = { 0 };
	if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return cpus;
	for (char* p = bus; *p; p++) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
	char path[160];
	snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/local_cpulist", bus);
	FILE* f = fopen(path, "r");
	if (!f) return cpus;
	char line[1024] = { 0 };
	if (fgets(line, (int)sizeof(line), f))
	{
		for (char* p = line; *p && *p != '\n'; )
		{
			char* end = nullptr;
			long a = strtol(p, &end, 10);
			if (end == p) break;
			long bnd = a;
			p = end;
			if (*p == '-') { bnd = strtol(p + 1, &end, 10); p = end; }
			for (long c = a; c <= bnd && c < 4096; c++) cpus.push_back((int)c);
			if (*p == ',') p++;
		}
	}
	fclose(f);
	return cpus;
}

/* Called on a shard's worker thread (never on the caller's own thread: its affinity is the caller's business).
 * ASTCENC_AMD_NUMA_BIND=0 switches it off. */
static void bind_worker_to_device(const DeviceSlot* s)
{
	static const bool enabled = []() { const char* e = getenv("ASTCENC_AMD_NUMA_BIND"); return !(e && e[0] == '0'); }();
	if (!enabled || s->local_cpus.empty()) return;
	cpu_set_t allowed, want;
	CPU_ZERO(&want);
	if (sched_getaffinity(0, sizeof(allowed), &allowed) != 0) return;
	int n = 0;
	for (int c : s->local_cpus) if (c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) { CPU_SET(c, &want); n++; }
	if (n > 0) (void)sched_setaffinity(0, sizeof(want), &want);        // (best effort: a container may forbid it)
}

/* Hands `task` to the slot's parked thread (started on first use, bound to the device's CPUs once); false when no
 * thread can be had -- std::system_error must not cross the C ABI --, or when the thread is busy with another call on
 * the same context (a second call used to wait here for the first call's whole shard before it even started its
 * own first one): the call then deals that device's share to the others (deal_portions).  The worker stays locked (w->mu)
 * until worker_wait(). */
static bool worker_run(DeviceSlot* s, std::function<void()> task)
{
	SlotWorker* w = s->worker;
	if (!w) return false;
	if (!w->mu.try_lock()) return false;
	if (!w->started)
	{
		try
		{
			w->thread = std::thread([w, s]()
			{
				bind_worker_to_device(s);
				std::unique_lock<std::mutex> lk(w->state_mu);
				for (;;)
				{
					w->wake.wait(lk, [w]() { return w->has_task || w->quit; });
					if (w->quit) return;
					std::function<void()> t = std::move(w->task);
					w->has_task = false;
					lk.unlock();
					t();
					lk.lock();
					w->done = true;
					w->done_cv.notify_all();
				}
			});
			w->started = true;
		}
		catch (...) { w->mu.unlock(); return false; }
	}
	{
		std::lock_guard<std::mutex> g(w->state_mu);
		w->task = std::move(task);
		w->has_task = true;
		w->done = false;
	}
	w->wake.notify_one();
	return true;
}
static void worker_wait(DeviceSlot* s)
{
	SlotWorker* w = s->worker;
	{
		std::unique_lock<std::mutex> lk(w->state_mu);
		w->done_cv.wait(lk, [w]() { return w->done; });
	}
	w->mu.unlock();
}

/* One slot on `device`: uploads the tables, sets the kernels' dynamic-LDS attribute there, creates streams
 * and events.  Every failure leaves through slot_destroy (the record starts zeroed). status: 1 = out of
 * memory, 2 = anything else. */
DeviceSlot* slot_create(Backend* b, int device, int* status)
{
	DeviceSlot* s = new DeviceSlot();
	s->device = device;
#define SLOT_TRY(expr, code) HIP_TRY(expr, { slot_destroy(s); *status = code; return nullptr; })
	SLOT_TRY(hipSetDevice(device), 2);
	{
		uint8_t layout[CTX_LAYOUT_BACK - CTX_CONFIG_BACK]; uint32_t layout_bytes = 0, lds_bytes = 0;
		int prc = kernel_prepare(b, &lds_bytes, layout, &layout_bytes);
		if (prc != 0)
		{
			log_msg("kernel setup failed on device %d (hip error %d)", device, prc);
			slot_destroy(s); *status = 2; return nullptr;
		}
	}
	SLOT_TRY(hipMalloc(&s->d_base, b->full.size() + ALLOC_SLACK), 1);
	SLOT_TRY(hipMemcpy(s->d_base, b->full.data(), b->full.size(), hipMemcpyHostToDevice), 2);
	s->d_tab = s->d_base + CTX_LAYOUT_BACK;
	s->d_dectab = s->d_base + b->dectab_offset;
	s->d_srgb = reinterpret_cast<const double*>(s->d_base + b->srgb_offset);
	SLOT_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), 2);
	SLOT_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking), 2);
	SLOT_TRY(hipEventCreateWithFlags(&s->ev_copy[0], hipEventDisableTiming), 2);
	SLOT_TRY(hipEventCreateWithFlags(&s->ev_copy[1], hipEventDisableTiming), 2);
	SLOT_TRY(hipEventCreateWithFlags(&s->ev_band, hipEventDisableTiming), 2);
	for (int i = 0; i < 3; i++) SLOT_TRY(hipEventCreateWithFlags(&s->ev_done[i], hipEventDisableTiming), 2);
	for (int i = 0; i < 2; i++) SLOT_TRY(hipEventCreateWithFlags(&s->ev_out[i], hipEventDisableTiming), 2);
	SLOT_TRY(hipEventCreate(&s->ev0), 2);
	SLOT_TRY(hipEventCreate(&s->ev1), 2);
	SLOT_TRY(hipEventCreate(&s->ev_gen), 2);
	SLOT_TRY(hipEventCreateWithFlags(&s->ev_tickets, hipEventDisableTiming), 2);
	SLOT_TRY(hipMalloc(reinterpret_cast<void**>(&s->d_tickets), TICKET_BUFFER_BYTES), 1);
#if defined(ASTC_PROFILE)
	enum { PS_COUNT = 40 };
	SLOT_TRY(hipMalloc(&s->d_prof, 2 * PS_COUNT * sizeof(unsigned long long)), 1);
	SLOT_TRY(hipMemset(s->d_prof, 0, 2 * PS_COUNT * sizeof(unsigned long long)), 2);
#endif
#undef SLOT_TRY
	s->local_cpus = device_local_cpus(device);
	slot_adopt_jit(b, s);      // (a slot created after the build arrived: devices joined on first use)
	*status = 0;
	return s;
}

/* Device list of a context.  Default: the calling thread's current device only (a rank-per-GPU process must not
 * initialise, or contend for, its neighbours' GPUs).  The N-device split of host images is opt-in:
 * ASTCENC_AMD_DEVICES = "all" (every visible device, the current one first) or a comma separated list of device
 * ordinals; an ordinal may repeat ("0,0": two slots on one GPU, which is how the multi-device path is tested on a
 * one-GPU box). */
std::vector<int> device_list(int ndev)
{
	std::vector<int> out;
	const char* env = getenv("ASTCENC_AMD_DEVICES");
	const bool all = env && strcmp(env, "all") == 0;
	if (env && *env && !all)
	{
		const char* p = env;
		while (*p)
		{
			char* e = nullptr;
			long v = strtol(p, &e, 10);
			if (e == p) break;
			if (v >= 0 && v < ndev) out.push_back((int)v);
			else log_msg("ASTCENC_AMD_DEVICES names device %ld, %d visible; ignored", v, ndev);
			p = e;
			while (*p == ',' || *p == ' ') p++;
		}
	}
	if (out.empty())
	{
		// current device first, so that a one-device caller keeps what it had selected
		int cur = 0;
		if (hipGetDevice(&cur) != hipSuccess) cur = 0;
		out.push_back(cur);
		if (all) for (int d = 0; d < ndev; d++) if (d != cur) out.push_back(d);
	}
	return out;
}

/* Slot that owns `ptr` (device memory); slot 0 when the runtime does not know the pointer. */
DeviceSlot* slot_for_pointer(Backend* b, const void* ptr, int* status)
{
	*status = 0;
	hipPointerAttribute_t attr;
	memset(&attr, 0, sizeof(attr));
	if (!ptr || hipPointerGetAttributes(&attr, ptr) != hipSuccess)
	{
		(void)hipGetLastError();
		return b->slots[0];
	}
	for (DeviceSlot* s : b->slots) if (s->device == attr.device) return s;     // (immutable after backend_create: no lock)
	std::lock_guard<std::mutex> lk(b->slots_mu);
	for (DeviceSlot* s : b->extra) if (s->device == attr.device) return s;
	DeviceSlot* s = slot_create(b, attr.device, status);
	if (s) b->extra.push_back(s);
	return s;
}

/* The stream a device-resident call runs on: the caller's, which must belong to the device the buffers (and the
 * slot's tables) live on, or the slot's own.  Returns false (-> rc 3, a bad argument) on a foreign stream. */
bool pick_stream(const DeviceSlot* s, void* caller_stream, hipStream_t* out)
{
	*out = s->stream;
	if (!caller_stream) return true;
	hipStream_t stream = static_cast<hipStream_t>(caller_stream);
	hipDevice_t sdev = -1;
	if (hipStreamGetDevice(stream, &sdev) != hipSuccess) { (void)hipGetLastError(); sdev = s->device; }
	if ((int)sdev != s->device)
	{
		log_msg("the stream belongs to device %d, the buffers to device %d", (int)sdev, s->device);
		return false;
	}
	*out = stream;
	return true;
}

/* Image sets.  Every buffer of the set must live on the device that owns entry 0's first buffer (or be unknown to the runtime,
 * which the single-image path allows as well); otherwise rc 3 and nothing is launched. */
bool set_on_one_device(const DeviceSlot* s, const void* const* ptrs, size_t count)
{
	for (size_t i = 0; i < count; i++)
	{
		hipPointerAttribute_t attr;
		memset(&attr, 0, sizeof(attr));
		if (!ptrs[i] || hipPointerGetAttributes(&attr, ptrs[i]) != hipSuccess) { (void)hipGetLastError(); continue; }
		if (attr.device != s->device)
		{
			log_msg("image set entry %zu: a buffer of device %d, entry 0's are on device %d", i / 2, attr.device, s->device);
			return false;
		}
	}
	return true;
}

/* Runs body(s, stream) with slot `s` locked and its device current, on the caller's stream (rc 3 if it is another device's) or
 * the slot's own. */
template <class Body> int run_locked(DeviceSlot* s, void* caller_stream, Body body)
{
	std::lock_guard<std::mutex> busy(s->busy);
	HIP_TRY(hipSetDevice(s->device), return 2);
	hipStream_t stream;
	if (!pick_stream(s, caller_stream, &stream)) return 3;
	return body(s, stream);
}

/* The setup of a call on device-resident buffers: run_locked on the slot that owns `owner` (a missing slot: the status of
 * slot_for_pointer, or 2), once the `count` pointers at `same_device` are known to be on its device as well (else rc 3). */
template <class Body> int run_on_owner(Backend* b, const void* owner, const void* const* same_device, size_t count, void* caller_stream, Body body)
{
	DeviceGuard guard;
	int st = 0;
	DeviceSlot* s = slot_for_pointer(b, owner, &st);
	if (!s) return st ? st : 2;
	if (!set_on_one_device(s, same_device, count)) return 3;
	return run_locked(s, caller_stream, body);
}

/* The decode launch of the image of `job` (a DecompressJob or DecompressDeviceJob) on slot `s`. */
template <class Job> DecodeLaunch decode_launch(const Backend* b, const DeviceSlot* s, const Job& job, const uint8_t* d_blocks, void* d_image, hipStream_t stream)
{
	DecodeLaunch d;
	d.d_blocks = d_blocks;
	d.d_image = d_image;
	d.d_tables = s->d_dectab;
	d.dim_x = job.dim_x; d.dim_y = job.dim_y; d.dim_z = job.dim_z ? job.dim_z : 1u; d.data_type = job.data_type;
	for (int i = 0; i < 4; i++) d.swz[i] = job.swz[i];
	d.block_x = b->root.dim_x; d.block_y = b->root.dim_y; d.block_z = b->root.dim_z;
	d.profile = b->cfg.profile;
	d.stream = stream;
	return d;
}

/* Completed-block counter shared by the slots of one call; the callback sees a monotonic percentage
 * (ref: ParallelManager::complete_task_assignment, astcenc_internal_entry.h:255-290). */
struct Progress {
	std::mutex mu;
	size_t done, total;
	void (*callback)(float);
	void add(size_t n)
	{
		if (!callback) return;
		std::lock_guard<std::mutex> lk(mu);
		done += n;
		callback(100.0f * (float)done / (float)total);
	}
};

} // namespace

Backend* backend_create(const uint8_t* blob, size_t blob_bytes, const DeviceConfig& cfg, int* status)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
	{
		log_msg("no HIP device available; this library has no CPU fallback");
		*status = 2;
		return nullptr;
	}
	DeviceGuard guard;

	Backend* b = new Backend;
	b->cfg = cfg;
	memcpy(&b->root, blob, sizeof(TableRoot));
	b->hdr = cfg.profile >= 2;
	b->lds_bytes = 0;
	b->variant = -1;
	b->jit = nullptr; b->jit_mode = JIT_OFF; b->blocks_done.store(0); b->jit_active.store(false);
	b->jit_lazy_blocks = JIT_LAZY_BLOCKS;
	// (ASTCENC_AMD_JIT_LAZY_BLOCKS: another trigger count -- tests/test_jit.py watches the background compile take over)
	if (const char* e = getenv("ASTCENC_AMD_JIT_LAZY_BLOCKS")) { const long long v = strtoll(e, nullptr, 10); if (v >= 1) b->jit_lazy_blocks = (unsigned long long)v; }
	uint8_t layout[CTX_LAYOUT_BACK - CTX_CONFIG_BACK];
	uint32_t layout_bytes = 0;
	{
		// layout record of the block's LDS working set (the kernels' dynamic-LDS attribute is per device: slot_create)
		int prc = kernel_prepare(b, &b->lds_bytes, layout, &layout_bytes);
		if (prc != 0)
		{
			log_msg("kernel setup failed (hip error %d)", prc);
			delete b; *status = 2; return nullptr;
		}
	}
	if (b->lds_bytes > 160 * 1024)
	{
		log_msg("block working set %u B; a CU has 160 KiB of LDS", b->lds_bytes);
		delete b; *status = 2; return nullptr;
	}

	// device allocation = [LdsLayout, 256 B][DeviceConfig, 256 B][table blob][decoder tables][sRGB tables of mip generation];
	// kernels get the blob pointer
	b->dectab_offset = (CTX_LAYOUT_BACK + blob_bytes + 255) & ~(size_t)255;
	b->srgb_offset = (b->dectab_offset + astc_decode_tables_bytes() + 255) & ~(size_t)255;
	b->full.assign(b->srgb_offset + astc_mip_srgb_table_bytes(), 0);
	astc_decode_tables_build(b->full.data() + b->dectab_offset, b->root.dim_x, b->root.dim_y, b->root.dim_z);
	astc_mip_srgb_tables_build(b->full.data() + b->srgb_offset);
	memcpy(b->full.data(), layout, layout_bytes);
	static_assert(sizeof(DeviceConfig) <= 256, "DeviceConfig outgrew its slot");
	memcpy(b->full.data() + (CTX_LAYOUT_BACK - CTX_CONFIG_BACK), &b->cfg, sizeof(DeviceConfig));
	memcpy(b->full.data() + CTX_LAYOUT_BACK, blob, blob_bytes);

#if !defined(ASTC_TRACE) && !defined(ASTC_DUPSTAGE) && !defined(ASTC_PROFILE) && !defined(ASTC_LDS_PAD_ENV)
	// A context that none of the library's fixed-context builds serves gets its own (kernel_jit.h): found in the disk cache,
	// or compiled in the background -- by default once the context has shown that it is used for more than a thumbnail.
	{
		const char* want = getenv("ASTCENC_AMD_KERNEL");
		b->jit_mode = want && strcmp(want, "generic") == 0 ? JIT_OFF : jit_mode_from_environment();
		if (b->jit_mode != JIT_OFF && !kernel_variants[b->variant].fixed)
		{
			int dev = 0;
			hipDeviceProp_t prop;
			if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
				b->jit = jit_acquire(layout, layout_bytes, b->cfg, b->root, b->hdr, prop.gcnArchName, [](const char* line) { log_msg("%s", line); });
			if (b->jit && b->jit_mode == JIT_EAGER) jit_start(b->jit);
			if (b->jit && b->jit_mode == JIT_SYNC) (void)jit_wait(b->jit);
		}
	}
#endif
	for (int device : device_list(ndev))
	{
		int st = 0;
		DeviceSlot* s = slot_create(b, device, &st);
		if (!s)
		{
			if (b->slots.empty()) { jit_release(b->jit); delete b; *status = st; return nullptr; }
			log_msg("device %d not usable, continuing with %zu device(s)", device, b->slots.size());
			continue;
		}
		// (every device but the first gets its parked host thread: the record here, the thread itself on first use)
		if (!b->slots.empty()) s->worker = new (std::nothrow) SlotWorker();
		b->slots.push_back(s);
	}
	*status = 0;
	return b;
}

void backend_destroy(Backend* b)
{
	if (!b) return;
	DeviceGuard guard;
	for (DeviceSlot* s : b->slots) slot_destroy(s);
	for (DeviceSlot* s : b->extra) slot_destroy(s);
	jit_release(b->jit);
	delete b;
}

int backend_device_count(const Backend* b) { return (int)b->slots.size(); }
const char* backend_kernel_name(const Backend* b)
{
	if (b->jit && b->jit_active.load()) return jit_kernel_name(b->jit);
	return b->variant >= 0 ? kernel_variants[b->variant].name : "";
}

int backend_specialize(Backend* b)
{
	if (b->variant >= 0 && kernel_variants[b->variant].fixed) return 0;
	if (!b->jit || jit_wait(b->jit) != JIT_READY) return 1;
	DeviceGuard guard;
	for (DeviceSlot* s : b->slots)
	{
		std::lock_guard<std::mutex> busy(s->busy);
		if (hipSetDevice(s->device) == hipSuccess) slot_adopt_jit(b, s);
	}
	return b->jit_active.load() ? 0 : 1;
}

/* The context's run-time build: adopted as soon as the compiler has delivered it; asked for (JIT_LAZY) once the context has
 * compressed enough to be worth a compile.  Called by every compression of `nblocks` blocks on slot `s`. */
static void jit_count_blocks(Backend* b, DeviceSlot* s, size_t nblocks)
{
	slot_adopt_jit(b, s);
	if (b->jit && b->jit_mode == JIT_LAZY && b->blocks_done.fetch_add(nblocks) + nblocks >= b->jit_lazy_blocks) jit_start(b->jit);
}

/* The alpha-average pre-pass of one image (`rows` texel rows of dim_x, dim_z slices) into d_averages.  Returns 0 ok, 1 out of
 * memory (or a radius whose scratch is refused), 2 launch failure.  alpha_scratch_release() once the call's pre-passes are queued. */
static int alpha_prepass(DeviceSlot* s, hipStream_t stream, const void* d_image, float* d_averages, uint32_t dim_x, uint32_t rows,
                         uint32_t dim_z, uint32_t data_type, uint32_t swz_a, uint32_t radius)
{
	AlphaLaunch a;
	a.d_image = d_image; a.d_averages = d_averages;
	a.dim_x = dim_x; a.dim_y = rows; a.dim_z = dim_z; a.data_type = data_type;
	a.swz_a = swz_a; a.radius = radius; a.stream = stream;
	a.d_scratch = nullptr; a.scratch_workgroups = 0;
	const size_t scratch = astc_alpha_scratch_bytes(dim_x, rows, dim_z, radius, &a.scratch_workgroups);
	if (scratch == (size_t)-1)
	{
		log_msg("a_scale_radius %u needs more than 1 GiB of pre-pass scratch per tile: refused", radius);
		return 1;
	}
	if (scratch)
	{
		if (grow(s->d_alpha_scratch, s->alpha_scratch_cap, scratch) != 0) return 1;
		a.d_scratch = s->d_alpha_scratch;
	}
	int arc = astc_alpha_launch(a);
	if (arc != 0) { log_msg("alpha pre-pass launch failed (hip error %d)", arc); return 2; }
	return 0;
}

/* (a large scratch is not kept for the life of the context: the pre-pass runs once per call, its scratch goes back as soon as
 *  the stream is past the kernel -- hipFree waits for that) */
static void alpha_scratch_release(DeviceSlot* s, hipStream_t stream)
{
	if (s->alpha_scratch_cap > ((size_t)64 << 20))
	{
		(void)hipStreamSynchronize(stream);
		(void)hipFree(s->d_alpha_scratch);
		s->d_alpha_scratch = nullptr; s->alpha_scratch_cap = 0;
	}
}

/* The kernel launches of one call: blocks [0, nblocks) of `k` (one image, or an image set's table) in chunks of `chunk`.
 * Chunks bound the time between cancel checks / progress callbacks on huge images; a chunk is still tens of thousands of
 * workgroups, far more than the 256 CUs need to stay full.  The host stays at most two chunks ahead of the device: chunk k-1's
 * completion event is waited for (and reported to the progress callback) after chunk k has been queued, so the device always
 * has its next kernel waiting, a cancel takes effect within two chunks, and nothing synchronises a whole stream.  The banded
 * host-pointer path does its own waiting in its two hooks.  After the call: `launched` blocks are queued, the last chunk
 * (`prev_blocks` of them) is neither waited for nor reported. */
struct ChunkLoop {
	KernelLaunch k;                   // every field but first / count
	size_t nblocks, chunk;
	bool chunked;                     // wait for and report every chunk
	bool timed;                       // ev0 / ev1 around the launches (kernel_ms)
	const std::atomic<int>* cancel_flag;
	Progress* progress;
	std::function<int(size_t first, size_t n)> before_launch;                                       // banded: 0 ok
	std::function<int(size_t first, size_t n, size_t chunk_index, size_t prev_blocks)> after_launch; // banded: 0 ok
	size_t launched, prev_blocks;
};

static int run_chunks(const Backend* b, DeviceSlot* s, ChunkLoop& L)
{
	const hipStream_t stream = static_cast<hipStream_t>(L.k.stream);
	if (L.timed) HIP_TRY(hipEventRecord(s->ev0, stream), return 2);
	L.launched = 0; L.prev_blocks = 0;
	size_t chunk_index = 0;
	for (size_t first = 0; first < L.nblocks; first += L.chunk, chunk_index++)
	{
		if (L.cancel_flag && L.cancel_flag->load(std::memory_order_relaxed)) break;
		size_t n = L.nblocks - first < L.chunk ? L.nblocks - first : L.chunk;
		if (L.before_launch && L.before_launch(first, n) != 0) return 2;
		KernelLaunch k = L.k;
		k.first = (uint32_t)first; k.count = (uint32_t)n;
		// more blocks than the device holds workgroups: that many workgroups draw the blocks from tickets (block_tickets.h)
		const long forced = compress_grid_from_env();
		uint32_t grid = 0;
		if (forced > 0) grid = (uint32_t)((size_t)forced < n ? (size_t)forced : n);
		else if (forced < 0) { const uint32_t resident = compress_grid(b, s); if (resident && n > resident) grid = resident; }
		if (grid && tickets_arm(s, k, grid) != 0) return 2;
		int lrc = kernel_launch(b, s, k);
		if (lrc != 0) { log_msg("kernel launch failed (hip error %d)", lrc); return 2; }
		if (grid && tickets_launched(s, k) != 0) return 2;
		L.launched = first + n;
		if (L.after_launch)
		{
			if (L.after_launch(first, n, chunk_index, L.prev_blocks) != 0) return 2;
		}
		else if (L.chunked)
		{
			HIP_TRY(hipEventRecord(s->ev_done[chunk_index % 3], stream), return 2);
			if (chunk_index > 0)
			{
				HIP_TRY(hipEventSynchronize(s->ev_done[(chunk_index - 1) % 3]), return 2);
				if (L.progress) L.progress->add(L.prev_blocks);
			}
		}
		L.prev_blocks = n;
	}
	if (L.timed) HIP_TRY(hipEventRecord(s->ev1, stream), return 2);
	return 0;
}

static int compress_pipeline(Backend* b, DeviceSlot* s, hipStream_t stream, const CompressJob& job, Progress* progress);

/* The blocks of `job` on slot `s` (a body of run_locked).  Returns 0 ok, 1 out of memory, 2 device failure. */
static int compress_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const CompressJob& job, Progress* progress)
{
	const int rc = compress_pipeline(b, s, stream, job, progress);
	if (rc != 0)
	{
		// A failed call may leave asynchronous copies of the banded pipeline in flight that read or write the pinned
		// staging buffers; the next call refills (or regrows and frees) those buffers without waiting for band 0 and 1.
		// Drain both streams before anybody can get there (best effort: the device may be the thing that failed).
		(void)hipStreamSynchronize(s->copy_stream);
		(void)hipStreamSynchronize(s->stream);
	}
	return rc;
}

static int compress_pipeline(Backend* b, DeviceSlot* s, hipStream_t stream, const CompressJob& job, Progress* progress)
{
	const BlockGrid grid = block_grid(b->root, job);
	const uint32_t bsy = b->root.dim_y, dim_z = grid.dim_z, blocks_x = grid.x, blocks_y = grid.y;
	// (a block list: the launches cover the positions of the list, everything else is the whole image's)
	const size_t nblocks = job.device_list ? (size_t)job.list_count : grid.count();
	jit_count_blocks(b, s, nblocks);
	const size_t row_bytes = (size_t)job.dim_x * texel_bytes(job.data_type);
	// (a shard of the alpha-scale split carries halo rows around its own: they are uploaded and averaged, not compressed)
	const uint32_t halo_above = dim_z == 1 && job.a_scale_radius != 0 ? job.halo_above : 0u;
	const uint32_t halo_below = dim_z == 1 && job.a_scale_radius != 0 ? job.halo_below : 0u;
	const uint32_t rows_with_halo = job.dim_y + halo_above + halo_below;
	const size_t slice_bytes = rows_with_halo * row_bytes;
	const size_t image_bytes = slice_bytes * dim_z;
	const size_t out_bytes = grid.count() * 16;

	const void* d_image = job.device_data;
	uint8_t* d_out = job.device_out;

	if (job.host_slices)
	{
		if (grow(s->d_image, s->image_cap, image_bytes) != 0) return 1;
		d_image = s->d_image;
	}
	// Host-pointer calls on a plain 2D image are pipelined by bands of block rows: band k+1 travels over
	// PCIe on the copy stream while band k is being compressed, and band k's blocks travel back while band
	// k+1 runs (a block only reads texel rows of its own band).  The alpha-scale pre-pass and volumes need
	// the whole image first.
	const bool banded = job.host_slices && job.host_out && dim_z == 1 && job.a_scale_radius == 0;
	if (job.host_slices && !banded)
	{
		for (uint32_t z = 0; z < dim_z; z++)
			HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(s->d_image) + z * slice_bytes, job.host_slices[z], slice_bytes, hipMemcpyHostToDevice, stream), return 2);
	}
	if (job.host_out)
	{
		if (grow(s->d_out, s->out_cap, out_bytes) != 0) return 1;
		d_out = s->d_out;
	}
	if (!d_image || !d_out) return 2;

	ImageDesc img = image_desc(b->root, b->cfg.profile, job, static_cast<const uint8_t*>(d_image) + halo_above * row_bytes);
	if (job.a_scale_radius != 0)
	{
		if (grow(s->d_alpha, s->alpha_cap, (size_t)job.dim_x * rows_with_halo * sizeof(float)) != 0) return 1;
		const int arc = alpha_prepass(s, stream, d_image, s->d_alpha, job.dim_x, rows_with_halo, dim_z, job.data_type, job.swz[3], job.a_scale_radius);
		if (arc != 0) return arc;
		img.alpha_avg = s->d_alpha + (size_t)halo_above * job.dim_x;
		alpha_scratch_release(s, stream);
	}

	// (chunks: run_chunks)
	const bool chunked = (progress && progress->callback) || job.host_slices;
	size_t chunk = chunked ? (size_t)1 << 18 : nblocks;
	if (banded)
	{
		// whole block rows per band; at least four bands when the image is large enough for a band to fill the device.  (A
		// block takes 0.8 ms from load to store whatever runs beside it -- its own instruction stream on one wave -- so a
		// kernel over a band is never shorter than that: four bands of a 256 x 256 image were four times 0.8 ms one after
		// the other, 3.4 ms for a call whose one launch takes 0.9; below BAND_MIN_BLOCKS the image is one band.)
		size_t rows = chunk / blocks_x;
		if (rows * 4 > blocks_y) rows = nblocks >= BAND_MIN_BLOCKS ? (blocks_y + 3) / 4 : blocks_y;
		if (rows < 1) rows = 1;
		chunk = rows * blocks_x;
	}
	if (banded)
	{
		// Pinned staging: a copy from or to the caller's pageable memory would hold the host thread until it is done (and the
		// D2H one until the band's kernel is done), so the device would sit idle while the next band is queued.  The host
		// copies a band into a pinned buffer (two of them: band k+1 is staged while band k's transfer is in flight) and the
		// blocks come back through pinned buffers as well; every transfer is then a true asynchronous DMA.
		const size_t band_rows = (chunk / blocks_x) * bsy;
		if (grow_pinned(s->h_in, s->h_in_cap, band_rows * row_bytes) != 0 || grow_pinned(s->h_out, s->h_out_cap, chunk * 16) != 0) return 1;
	}
	auto upload_band = [&](size_t band_first, size_t band_blocks) -> int {
		const size_t band = band_first / chunk;
		const size_t y0 = (band_first / blocks_x) * bsy;
		size_t y1 = ((band_first + band_blocks) / blocks_x) * bsy;
		if (y1 > job.dim_y) y1 = job.dim_y;
		// the staging buffer's previous transfer (band - 2) must have left it
		if (band >= 2) HIP_TRY(hipEventSynchronize(s->ev_copy[band & 1]), return 2);
		memcpy(s->h_in[band & 1], static_cast<const uint8_t*>(job.host_slices[0]) + y0 * row_bytes, (y1 - y0) * row_bytes);
		HIP_TRY(hipMemcpyAsync(static_cast<uint8_t*>(s->d_image) + y0 * row_bytes, s->h_in[band & 1], (y1 - y0) * row_bytes, hipMemcpyHostToDevice, s->copy_stream), return 2);
		HIP_TRY(hipEventRecord(s->ev_copy[band & 1], s->copy_stream), return 2);
		return 0;
	};
	// a band's blocks, once its transfer has landed in the pinned buffer, go to the caller's memory (and to the progress count)
	auto collect_band = [&](size_t band_first, size_t band_blocks) -> int {
		const size_t band = band_first / chunk;
		HIP_TRY(hipEventSynchronize(s->ev_out[band & 1]), return 2);
		memcpy(job.host_out + band_first * 16, s->h_out[band & 1], band_blocks * 16);
		if (progress) progress->add(band_blocks);
		return 0;
	};
#if defined(ASTC_TRACE)
	{
		// debug build: one trace slice per block, dumped to $ASTCENC_AMD_TRACE_FILE after the call (wave_ctx.h: TRACE_PUT)
		const size_t need = grid.count() * TRACE_WORDS_PER_BLOCK_HOST * sizeof(uint32_t);
		if (grow(s->d_prof, s->trace_cap, need) != 0) return 1;
		HIP_TRY(hipMemsetAsync(s->d_prof, 0, need, stream), return 2);
	}
#endif
	ChunkLoop L;
	L.k.d_tab = s->d_tab; L.k.lds_bytes = b->lds_bytes; L.k.img = img; L.k.d_out = d_out;
	L.k.stream = stream; L.k.d_prof = s->d_prof; L.k.d_set = nullptr;
	L.nblocks = nblocks; L.chunk = chunk; L.chunked = chunked; L.timed = job.kernel_ms != nullptr;
	L.cancel_flag = job.cancel_flag; L.progress = progress;
	if (banded)
	{
		L.before_launch = [&](size_t first, size_t n) -> int {
			// band 0 first; from then on the next band is queued before this band's kernel, so that it
			// crosses PCIe while the kernel runs (and ahead of this band's results on the copy stream)
			if (first == 0 && upload_band(0, n) != 0) return 2;
			const size_t next = first + n;
			if (next < nblocks && upload_band(next, nblocks - next < chunk ? nblocks - next : chunk) != 0) return 2;
			HIP_TRY(hipStreamWaitEvent(stream, s->ev_copy[(first / chunk) & 1], 0), return 2);
			return 0;
		};
		L.after_launch = [&](size_t first, size_t n, size_t chunk_index, size_t prev_blocks) -> int {
			// this band's blocks go home on the copy stream once its kernel is done; the band before it is collected
			// meanwhile (its transfer was queued one iteration ago, behind its own kernel)
			HIP_TRY(hipEventRecord(s->ev_band, stream), return 2);
			HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_band, 0), return 2);
			HIP_TRY(hipMemcpyAsync(s->h_out[chunk_index & 1], d_out + first * 16, n * 16, hipMemcpyDeviceToHost, s->copy_stream), return 2);
			HIP_TRY(hipEventRecord(s->ev_out[chunk_index & 1], s->copy_stream), return 2);
			if (chunk_index > 0 && collect_band(first - prev_blocks, prev_blocks) != 0) return 2;
			return 0;
		};
	}
	if (run_chunks(b, s, L) != 0) return 2;
	const size_t launched = L.launched, prev_blocks = L.prev_blocks;

	if (job.host_out && !banded && launched)
	{
		// after a cancel only the blocks that were compressed go home; the rest of the caller's buffer stays untouched
		HIP_TRY(hipMemcpyAsync(job.host_out, d_out, launched * 16, hipMemcpyDeviceToHost, stream), return 2);
	}
	HIP_TRY(hipStreamSynchronize(stream), return 2);
	if (banded)
	{
		// the last band that was launched (after a cancel: the last one before it) is still on its way
		if (launched && collect_band(launched - prev_blocks, prev_blocks) != 0) return 2;
		HIP_TRY(hipStreamSynchronize(s->copy_stream), return 2);
	}
	else if (chunked && progress && prev_blocks && launched) progress->add(prev_blocks);
	if (job.kernel_ms) HIP_TRY(hipEventElapsedTime(job.kernel_ms, s->ev0, s->ev1), return 2);
#if defined(ASTC_TRACE)
	if (const char* path = getenv("ASTCENC_AMD_TRACE_FILE"))
	{
		std::vector<uint32_t> host(grid.count() * TRACE_WORDS_PER_BLOCK_HOST);
		HIP_TRY(hipMemcpy(host.data(), s->d_prof, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost), return 2);
		if (FILE* f = fopen(path, "wb")) { fwrite(host.data(), sizeof(uint32_t), host.size(), f); fclose(f); }
	}
#endif
#if defined(ASTC_PROFILE)
	{
		enum { PS_COUNT = 40, PS_TOTAL = 14 };
		static const char* names[PS_COUNT] = { "load", "ideal", "decimate", "angular", "modes", "formats", "recompute", "pack", "diff",
		                                        "realign", "kmeans+partsearch", "  partscore", "physical", "stats", "TOTAL", "blocks",
		                                        "  dec sweep1", "  dec infill", "  dec sweep3", "  ang phase1", "  ang phase2",
		                                        "  mode terms", "  mode acc", "  mode quant", "  fmt eci", "  fmt table", "  fmt combine", "  fmt select",
		                                        "  cand staging", "  physical", "  refine (all)", "  trial (all)",
		                                        "  y0 cand quantize", "  y1 cand setup", "  y2 after pack", "  y3 accept/copy", "  y4 realign infill", "  y5 realign undecimated", "  y6 realign lane-per-weight eval", "  y7 realign movers" };
		unsigned long long h[2 * PS_COUNT];
		HIP_TRY(hipMemcpy(h, s->d_prof, sizeof(h), hipMemcpyDeviceToHost), return 2);
		HIP_TRY(hipMemset(s->d_prof, 0, sizeof(h)), return 2);
		fprintf(stderr, "stage cycles per block (lane-0 shader clock), %zu blocks:   [calls per block]\n", nblocks);
		for (int i = 0; i < PS_COUNT; i++)
			if (i != 15 && h[i])
				fprintf(stderr, "  %-18s %12.0f  %5.1f%%   [%6.2f]\n", names[i], (double)h[i] / (double)nblocks, 100.0 * (double)h[i] / (double)h[PS_TOTAL],
				        (double)h[PS_COUNT + i] / (double)nblocks);
	}
#endif
	return 0;
}

/* Smallest shard worth a device of its own: below this a second GPU's fixed costs (its PCIe transfers start
 * later, its L2 has to fetch the tables again) outweigh the kernel time it takes over. */
constexpr size_t MIN_BLOCKS_PER_DEVICE = 16384;
/* Portions a sharded call is cut into per device (backend_compress): enough for a device that got cheap content to take
 * over work from one that did not, few enough for the pipeline restart at a portion's first band not to show. */
constexpr size_t DEAL_PORTIONS_PER_DEVICE = 4;
/* ... and a portion is at least this many blocks (a 2048^2 image at 6x6): every portion starts its PCIe pipeline anew -- its
 * first band crosses before anything is compressed -- which eight portions of 16 k blocks pay for visibly (profiles/r06z). */
constexpr size_t MIN_BLOCKS_PER_PORTION = 4 * MIN_BLOCKS_PER_DEVICE;

/* A 2D image is cut into block rows, a volume / stack of slices into layers of blocks. */
static uint32_t shard_units(const BlockGrid& grid) { return grid.dim_z == 1 ? grid.y : grid.z; }

/* How many of the context's devices a host image is shared out to. */
static size_t devices_for(const Backend* b, const BlockGrid& grid)
{
	size_t ndev = b->slots.size();
	const size_t by_size = grid.count() / MIN_BLOCKS_PER_DEVICE;
	if (ndev > by_size) ndev = by_size < 1 ? 1 : by_size;
	if (ndev > shard_units(grid)) ndev = shard_units(grid);
	return ndev;
}

static const void* advance(const void* p, size_t bytes) { return static_cast<const uint8_t*>(p) + bytes; }
static void* advance(void* p, size_t bytes) { return static_cast<uint8_t*>(p) + bytes; }

/* A contiguous range of a host image: whole block rows of a 2D image or whole block layers of a volume, blocks
 * [first_block, first_block + blocks) of the image.  `job` is the image's job cut down to the range (host_slices = slices, dim_y
 * or dim_z its own); the caller points it at the range's blocks. */
template <class Job> struct Shard {
	Job job;
	std::vector<std::decay_t<decltype(*std::declval<Job&>().host_slices)>> slices;   // (const void* / void*)
	uint32_t first_row;                // 2D: the range's first texel row
	size_t first_block, blocks;
};

/* The host image of `job` cut into at most `count` ranges of equal size (the last one shorter). */
template <class Job> static std::vector<Shard<Job>> cut_shards(const Backend* b, const BlockGrid& grid, const Job& job, size_t count)
{
	const uint32_t units = shard_units(grid), units_per = (uint32_t)((units + count - 1) / count);
	const size_t unit_blocks = grid.dim_z == 1 ? (size_t)grid.x : (size_t)grid.x * grid.y;
	const size_t row_bytes = (size_t)job.dim_x * texel_bytes(job.data_type);
	std::vector<Shard<Job>> shards;
	for (uint32_t u0 = 0; u0 < units; u0 += units_per)
	{
		const uint32_t u1 = u0 + units_per < units ? u0 + units_per : units;
		Shard<Job> sh;
		sh.job = job;
		sh.first_row = 0;
		sh.first_block = u0 * unit_blocks;
		sh.blocks = (u1 - u0) * unit_blocks;
		if (grid.dim_z == 1)
		{
			const uint32_t y0 = u0 * b->root.dim_y;
			const uint32_t y1 = u1 * b->root.dim_y < job.dim_y ? u1 * b->root.dim_y : job.dim_y;
			sh.first_row = y0;
			sh.slices.push_back(advance(job.host_slices[0], y0 * row_bytes));
			sh.job.dim_y = y1 - y0;
		}
		else
		{
			const uint32_t z0 = u0 * b->root.dim_z;
			const uint32_t z1 = u1 * b->root.dim_z < grid.dim_z ? u1 * b->root.dim_z : grid.dim_z;
			sh.slices.assign(job.host_slices + z0, job.host_slices + z1);
			sh.job.dim_z = z1 - z0;
		}
		shards.push_back(std::move(sh));
	}
	for (Shard<Job>& sh : shards) sh.job.host_slices = sh.slices.data();      // (after the vector stopped growing)
	return shards;
}

/* Runs portions 0 .. count - 1 of a host image as run(slot, portion) on the first `ndev` slots.  The portions are DEALT, not
 * pre-assigned: the calling thread drives slot 0, the parked thread of every further slot drives that one, and each takes the next
 * portion from one counter when it has finished its last.  A slot whose thread is busy with another call on the context or cannot
 * be had (std::system_error must not cross the C ABI, and the earlier workers must still be joined) takes no portions: the others
 * deal its share out.  A failed portion fails the call -- nobody starts another --; the first failure is returned, out of memory
 * before any other.  log_as: the name in the per-slot log line, or null for none. */
static int deal_portions(Backend* b, size_t ndev, size_t count, const std::function<int(DeviceSlot*, size_t)>& run, const char* log_as)
{
	std::vector<int> rcs(count, 0);
	std::atomic<size_t> next_portion{0};
	std::atomic<bool> failed{false};
	const size_t nslots = ndev < count ? ndev : count;
	std::vector<double> busy_ms(nslots, 0.0);
	std::vector<unsigned> taken(nslots, 0u);
	auto deal = [&](size_t g)
	{
		const auto t0 = std::chrono::steady_clock::now();
		for (;;)
		{
			if (failed.load()) break;
			const size_t p = next_portion.fetch_add(1);
			if (p >= count) break;
			rcs[p] = run(b->slots[g], p);
			if (rcs[p] != 0) failed.store(true);
			taken[g]++;
		}
		busy_ms[g] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	};
	std::vector<size_t> on_workers;
	for (size_t g = 1; g < nslots; g++)
	{
		// (building the task may allocate: nothing may be thrown across the C ABI -- ADVICE r05)
		try { if (worker_run(b->slots[g], [&deal, g]() { deal(g); })) on_workers.push_back(g); }
		catch (...) { }
	}
	deal(0);
	for (size_t g : on_workers) worker_wait(b->slots[g]);
	if (log_as)
		for (size_t g = 0; g < nslots; g++) log_msg("%s: device slot %zu took %u of %zu portions, busy %.2f ms", log_as, g, taken[g], count, busy_ms[g]);
	int rc = 0;
	for (int r : rcs) if (r != 0 && (rc == 0 || r == 1)) rc = r;
	return rc;
}

int backend_compress(Backend* b, const CompressJob& job)
{
	const BlockGrid grid = block_grid(b->root, job);
	Progress progress;
	progress.done = 0; progress.callback = job.progress; progress.total = job.device_list ? job.list_count : grid.count();

	// Buffers that already live on a device are compressed there (a block list must live there as well).
	const void* list_ptr[1] = { job.device_list };
	if (!job.host_slices)
		return run_on_owner(b, job.device_data, list_ptr, 1, job.stream, [&](DeviceSlot* s, hipStream_t stream) { return compress_on_slot(b, s, stream, job, &progress); });

	// Host images: contiguous ranges of block rows (2D) or of block layers (volumes, stacks of slices), one per device,
	// each running its own pipeline on its own streams from its own host thread; the caller's thread takes the first
	// shard and joins the rest (ref: the block loop of compress_image, astcenc_entry.cpp:1009-1038 -- blocks are
	// independent, so the split needs no exchange).  With the alpha-scale pre-pass (ref: the same split over the
	// worker threads, astcenc_entry.cpp:1190-1211, astcenc_compute_variance.cpp:507) a shard also takes the texel rows its
	// averages reach into: enough rows above and below for every 32 x 32 tile of the pre-pass that touches the shard to
	// see exactly the texels it sees in the whole image -- same tiles, same summed-area arithmetic, same floats.
	DeviceGuard guard;
	auto on_slot = [b, &progress](DeviceSlot* slot, const CompressJob& j)
	{
		return run_locked(slot, j.stream, [&](DeviceSlot* s, hipStream_t stream) { return compress_on_slot(b, s, stream, j, &progress); });
	};
	// (a stack of slices with the alpha-scale pre-pass averages around slice 0 for the whole stack: one device)
	size_t ndev = (job.a_scale_radius != 0 && grid.dim_z > 1) || !job.host_out ? 1 : devices_for(b, grid);
#if defined(ASTC_TRACE)
	ndev = 1;      // (debug build: every shard would write the same trace file)
#endif
	if (ndev <= 1) return on_slot(b->slots[0], job);

	// The units are DEALT, not pre-assigned (ref: the reference's workers take blocks from one atomic ticket counter, 16 at a
	// time, astcenc_internal_entry.h:225-236 / astcenc_entry.cpp:959 -- a worker that lands on cheap content takes more):
	// block cost depends on content (a photograph runs three times faster per texel than noise), so with one contiguous range
	// per device the device that got the hard part of the image sets the call's time.  The image is cut into portions --
	// DEAL_PORTIONS_PER_DEVICE per device, none below MIN_BLOCKS_PER_DEVICE blocks -- and every device's host thread takes
	// the next portion from one counter when it has finished its last; a portion runs the banded PCIe pipeline of the
	// single-device path, so consecutive bands still overlap inside it.  ASTCENC_AMD_DEAL=static: one portion per device.
	size_t nportions = ndev;
	{
		const char* deal = getenv("ASTCENC_AMD_DEAL");
		if (!(deal && strcmp(deal, "static") == 0))
		{
			nportions = ndev * DEAL_PORTIONS_PER_DEVICE;
			// (ASTCENC_AMD_DEAL_MIN_BLOCKS: a smaller minimum, for tests/test_multi_device.py -- many portions on a small image)
			size_t min_portion = MIN_BLOCKS_PER_PORTION;
			if (const char* e = getenv("ASTCENC_AMD_DEAL_MIN_BLOCKS")) { const long v = strtol(e, nullptr, 10); if (v >= 1) min_portion = (size_t)v; }
			const size_t by_portion_size = grid.count() / min_portion;
			if (nportions > by_portion_size) nportions = by_portion_size;
			if (nportions > shard_units(grid)) nportions = shard_units(grid);
			if (nportions < ndev) nportions = ndev;
		}
	}
	std::vector<Shard<CompressJob>> shards = cut_shards(b, grid, job, nportions);
	// The reference's fast loader reads slice 0 whatever the block's z (CompressJob::fast_load_slice0): a shard that
	// starts further up the stack must then see the image's first slice as its own first slice.
	const bool slice0_quirk = grid.dim_z > 1 && job.fast_load_slice0 && uses_fast_load(b->root, b->cfg.profile, job);
	for (Shard<CompressJob>& sh : shards)
	{
		sh.job.progress = nullptr;
		sh.job.host_out = job.host_out + sh.first_block * 16;
		if (slice0_quirk) for (const void*& slice : sh.slices) slice = job.host_slices[0];
		if (grid.dim_z == 1 && job.a_scale_radius != 0)
		{
			// tiles of the pre-pass start at multiples of ALPHA_TILE from the image origin; a tile's summed-area table
			// takes in radius + 1 rows above its first row and radius rows below its last
			const uint32_t y0 = sh.first_row, y1 = y0 + sh.job.dim_y;
			const uint32_t tile = ALPHA_TILE_ROWS_2D, r = job.a_scale_radius;
			const uint32_t tile_top = y0 / tile * tile, tile_bottom = (y1 + tile - 1) / tile * tile;
			const uint32_t want_top = tile_top > r + 1 ? (tile_top - (r + 1)) / tile * tile : 0u;
			const uint64_t want_bottom = (uint64_t)tile_bottom + r + 1;
			const uint32_t last_row = want_bottom < job.dim_y ? (uint32_t)want_bottom : job.dim_y;
			sh.job.halo_above = y0 - want_top;
			sh.job.halo_below = last_row - y1;
			sh.slices[0] = advance(job.host_slices[0], (size_t)want_top * job.dim_x * texel_bytes(job.data_type));
		}
	}
	return deal_portions(b, ndev, shards.size(), [&](DeviceSlot* s, size_t p) { return on_slot(s, shards[p].job); }, "compress");
}

/* The blocks of `job` decoded on slot `s` (a body of run_locked). */
static int decompress_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const DecompressJob& job)
{
	const uint32_t dim_z = job.dim_z ? job.dim_z : 1u;
	const size_t slice_bytes = (size_t)job.dim_x * job.dim_y * texel_bytes(job.data_type);
	// the staging buffers of the compress path are reused the other way round
	if (grow(s->d_image, s->image_cap, slice_bytes * dim_z) != 0 || grow(s->d_out, s->out_cap, job.block_bytes) != 0) return 1;
	HIP_TRY(hipMemcpyAsync(s->d_out, job.host_blocks, job.block_bytes, hipMemcpyHostToDevice, stream), return 2);
	int lrc = astc_decode_launch(decode_launch(b, s, job, s->d_out, s->d_image, stream));
	if (lrc != 0) { log_msg("decode kernel launch failed (hip error %d)", lrc); return 2; }
	for (uint32_t z = 0; z < dim_z; z++)
		HIP_TRY(hipMemcpyAsync(job.host_slices[z], static_cast<uint8_t*>(s->d_image) + z * slice_bytes, slice_bytes, hipMemcpyDeviceToHost, stream), return 2);
	HIP_TRY(hipStreamSynchronize(stream), return 2);
	return 0;
}

/* Host blocks -> host image.  Like compression the work is dealt to the context's devices in contiguous ranges --
 * block rows of a 2D image, layers of blocks of a volume -- each decoded into its own rows / slices of the caller's
 * image (ref: the block loop of astcenc_decompress_image, astcenc_entry.cpp:1340-1385: blocks are independent), one
 * portion per device. */
int backend_decompress(Backend* b, const DecompressJob& job)
{
	DeviceGuard guard;
	const BlockGrid grid = block_grid(b->root, job);
	auto on_slot = [b](DeviceSlot* slot, const DecompressJob& j)
	{
		return run_locked(slot, nullptr, [&](DeviceSlot* s, hipStream_t stream) { return decompress_on_slot(b, s, stream, j); });
	};
	const size_t ndev = devices_for(b, grid);
	if (ndev <= 1) return on_slot(b->slots[0], job);
	std::vector<Shard<DecompressJob>> shards = cut_shards(b, grid, job, ndev);
	for (Shard<DecompressJob>& sh : shards)
	{
		sh.job.host_blocks = job.host_blocks + sh.first_block * 16;
		sh.job.block_bytes = sh.blocks * 16;
	}
	return deal_portions(b, ndev, shards.size(), [&](DeviceSlot* s, size_t p) { return on_slot(s, shards[p].job); }, nullptr);
}

int backend_decompress_device(Backend* b, const DecompressDeviceJob& job)
{
	return run_on_owner(b, job.device_image, nullptr, 0, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		int lrc = astc_decode_launch(decode_launch(b, s, job, job.device_blocks, job.device_image, stream));
		if (lrc != 0) { log_msg("decode kernel launch failed (hip error %d)", lrc); return 2; }
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		return 0;
	});
}

int backend_compare(Backend* b, const CompareJob& job)
{
	return run_on_owner(b, job.device_a, nullptr, 0, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		if (!s->d_sums) HIP_TRY(hipMalloc(&s->d_sums, astc_compare_scratch_doubles() * sizeof(double)), return 1);
		CompareLaunch c;
		c.d_a = job.device_a; c.type_a = job.type_a; c.d_b = job.device_b; c.type_b = job.type_b;
		c.texels = job.texels; c.d_sums = s->d_sums; c.stream = stream;
		c.hdr = job.hdr; c.fstop_lo = job.fstop_lo; c.fstop_hi = job.fstop_hi;
		int lrc = astc_compare_launch(c);
		if (lrc != 0) { log_msg("compare kernel launch failed (hip error %d)", lrc); return 2; }
		HIP_TRY(hipMemcpyAsync(job.sums, s->d_sums, METRIC_SUMS_HOST * sizeof(double), hipMemcpyDeviceToHost, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		return 0;
	});
}

/* Grows the slot's table buffer to `bytes` and queues the upload of the host copy (s->h_set). */
static int set_table_upload(DeviceSlot* s, hipStream_t stream, size_t bytes)
{
	if (grow(s->d_set, s->set_cap, bytes) != 0) return 1;
	HIP_TRY(hipMemcpyAsync(s->d_set, s->h_set.data(), bytes, hipMemcpyHostToDevice, stream), return 2);
	return 0;
}

/* Queues the generation of a mip chain and its post-passes on `stream` (the slot's lock held).  The windowed filter's taps and
 * the post-passes' scratch are sized first: if they cannot be had, nothing is launched. */
static int generate_mips_locked(DeviceSlot* s, hipStream_t stream, const MipChainJob& job)
{
	if (job.filter_kind)
	{
		const int trc = astc_mip_filter_table_build(job, s->h_mip_filter);
		if (trc == 1) { log_msg("the mip filter's taps exceed the 64 MiB scratch bound"); return 1; }
		if (trc != 0) { log_msg("mip filter table: a tile's taps exceed the kernel's rows"); return 2; }
		if (grow(s->d_mip_filter, s->mip_filter_cap, s->h_mip_filter.size()) != 0) return 1;
	}
	const size_t post = job.post_flags ? astc_mip_post_scratch_bytes(job) : 0;
	if (post && grow(s->d_mip_post, s->mip_post_cap, post) != 0) return 1;
	if (job.filter_kind)
	{
		HIP_TRY(hipMemcpyAsync(s->d_mip_filter, s->h_mip_filter.data(), s->h_mip_filter.size(), hipMemcpyHostToDevice, stream), return 2);
		const int frc = job.filter_edge == MIP_EDGE_CUBE ? astc_mip_cube_launch(job, s->d_mip_filter, s->d_srgb, stream)
		                : job.weight ? astc_mip_filter_weighted_launch(job, s->d_mip_filter, s->d_srgb, stream)
		                : astc_mip_filter_launch(job, s->d_mip_filter, s->d_srgb, stream);
		if (frc != 0) { log_msg("mip filter kernel launch failed (hip error %d)", frc); return 2; }
	}
	else
	{
		const int lrc = job.weight ? astc_mip_weighted_launch(job, s->d_srgb, stream) : astc_mip_launch(job, s->d_srgb, stream);
		if (lrc != 0) { log_msg("mip generation kernel launch failed (hip error %d)", lrc); return 2; }
	}
	const int prc = astc_mip_post_launch(job, s->d_mip_post, stream);
	if (prc != 0) { log_msg("mip post-pass kernel launch failed (hip error %d)", prc); return 2; }
	return 0;
}

/* An image set on slot `s` (a body of run_locked). */
static int compress_set_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const CompressSetJob& job, Progress* progress)
{
	if (job.generate)
	{
		// the levels first (kernel_ms counts from here), then everything below reads them in stream order
		if (job.kernel_ms) HIP_TRY(hipEventRecord(s->ev_gen, stream), return 2);
		const int grc = generate_mips_locked(s, stream, *job.generate);
		if (grc != 0) return grc;
	}
	const uint32_t count = job.count;
	const size_t rec_offset = image_set_records_offset(count);
	const size_t table_bytes = rec_offset + (size_t)count * sizeof(ImageSetEntryDesc);
	s->h_set.assign(table_bytes, 0);
	uint32_t* first = reinterpret_cast<uint32_t*>(s->h_set.data() + image_set_first_offset());
	ImageSetEntryDesc* rec = reinterpret_cast<ImageSetEntryDesc*>(s->h_set.data() + rec_offset);
	// the entries' blocks back to back; the alpha averages of the entries that need them side by side in one buffer
	size_t nblocks = 0, alpha_floats = 0;
	std::vector<size_t> alpha_at(count, 0);
	for (uint32_t e = 0; e < count; e++)
	{
		const CompressJob& en = job.entries[e];
		rec[e].img = image_desc(b->root, b->cfg.profile, en, en.device_data);
		rec[e].out = en.device_out;
		first[e] = (uint32_t)nblocks;
		nblocks += (size_t)rec[e].img.blocks_x * rec[e].img.blocks_y * rec[e].img.blocks_z;
		if (en.a_scale_radius != 0)
		{
			alpha_at[e] = alpha_floats;
			alpha_floats += ((size_t)en.dim_x * en.dim_y + 63) & ~(size_t)63;
		}
	}
	if (nblocks > 0xFFFFFFFFu) return 3;
	ImageSetTable* t = reinterpret_cast<ImageSetTable*>(s->h_set.data());
	t->count = count;
	t->total = (uint32_t)nblocks;
	// (a block list: the launches cover the positions of the list, everything else is the whole set's)
	const size_t launch_blocks = job.device_list ? (size_t)job.list_count : nblocks;
	jit_count_blocks(b, s, launch_blocks);

	if (alpha_floats)
	{
		if (grow(s->d_alpha, s->alpha_cap, alpha_floats * sizeof(float)) != 0) return 1;
		for (uint32_t e = 0; e < count; e++)
		{
			const CompressJob& en = job.entries[e];
			if (en.a_scale_radius == 0) continue;
			const int arc = alpha_prepass(s, stream, en.device_data, s->d_alpha + alpha_at[e], en.dim_x, en.dim_y, rec[e].img.dim_z, en.data_type, en.swz[3], en.a_scale_radius);
			if (arc != 0) return arc;
			rec[e].img.alpha_avg = s->d_alpha + alpha_at[e];
		}
		alpha_scratch_release(s, stream);
	}
	const int urc = set_table_upload(s, stream, table_bytes);
	if (urc != 0) return urc;

	ChunkLoop L;
	L.k.d_tab = s->d_tab; L.k.lds_bytes = b->lds_bytes; L.k.img = rec[0].img; L.k.d_out = rec[0].out;
	L.k.stream = stream; L.k.d_prof = s->d_prof; L.k.d_set = reinterpret_cast<const ImageSetTable*>(s->d_set);
	if (job.device_list)
	{
		// the by-value record of a set launch carries the list, and as its block count the set's total: the kernel head bounds a
		// listed index by it before the index goes through the set's table (kernel_device.h)
		L.k.img.list = job.device_list;
		L.k.img.blocks_x = (uint32_t)nblocks; L.k.img.blocks_y = 1; L.k.img.blocks_z = 1;
	}
#if defined(ASTC_TRACE)
	L.k.d_prof = nullptr;      // (the search trace is a single-image debug aid: compress_on_slot_locked sizes its buffer)
#endif
	L.chunked = progress && progress->callback;
	L.nblocks = launch_blocks; L.chunk = L.chunked ? (size_t)1 << 18 : launch_blocks;
	L.timed = job.kernel_ms != nullptr;
	L.cancel_flag = job.cancel_flag; L.progress = progress;
	if (run_chunks(b, s, L) != 0) return 2;
	HIP_TRY(hipStreamSynchronize(stream), return 2);
	if (L.chunked && L.prev_blocks && L.launched) progress->add(L.prev_blocks);
	if (job.kernel_ms) HIP_TRY(hipEventElapsedTime(job.kernel_ms, job.generate ? s->ev_gen : s->ev0, s->ev1), return 2);
	return 0;
}

int backend_compress_set(Backend* b, const CompressSetJob& job)
{
	if (job.generate && job.generate->device_image != job.entries[0].device_data) return 3;
	std::vector<const void*> ptrs;
	for (uint32_t e = 0; e < job.count; e++) { ptrs.push_back(job.entries[e].device_data); ptrs.push_back(job.entries[e].device_out); }
	ptrs.push_back(job.device_list); ptrs.push_back(nullptr);
	Progress progress;
	progress.done = 0; progress.callback = job.progress; progress.total = 0;
	for (uint32_t e = 0; e < job.count; e++) progress.total += block_grid(b->root, job.entries[e]).count();
	if (job.device_list) progress.total = job.list_count;
	return run_on_owner(b, job.entries[0].device_data, ptrs.data(), ptrs.size(), job.stream, [&](DeviceSlot* s, hipStream_t stream) { return compress_set_on_slot(b, s, stream, job, &progress); });
}

int backend_decompress_set(Backend* b, const DecompressSetJob& job)
{
	std::vector<const void*> ptrs;
	for (uint32_t e = 0; e < job.count; e++) { ptrs.push_back(job.entries[e].device_image); ptrs.push_back(job.entries[e].device_blocks); }
	return run_on_owner(b, job.entries[0].device_image, ptrs.data(), ptrs.size(), job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		std::vector<DecodeLaunch> d(job.count);
		for (uint32_t e = 0; e < job.count; e++) d[e] = decode_launch(b, s, job.entries[e], job.entries[e].device_blocks, job.entries[e].device_image, nullptr);
		const size_t bytes = astc_decode_set_bytes(job.count);
		s->h_set.assign(bytes, 0);
		const uint32_t runs = astc_decode_set_build(s->h_set.data(), d.data(), job.count);
		const int urc = set_table_upload(s, stream, bytes);
		if (urc != 0) return urc;
		int lrc = astc_decode_set_launch(s->d_set, runs, stream);
		if (lrc != 0) { log_msg("decode kernel launch failed (hip error %d)", lrc); return 2; }
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		return 0;
	});
}

/* astcenc_amd_decompress_regions_device, astcenc_amd_decompress_tensors_device and astcenc_amd_decompress_scaled_tensors_device: as
 * backend_decompress_set, with the regions' table (decode_regions.h, decode_tensors.h, decode_scaled.h) in place of the set's.
 * Only the entries a region names (used[e]) are looked at; their streams and every region's buffer must be on the owner's device.
 * out_of: region i's buffer (with `buffers` of them a region, buffer i belongs to region i / buffers); table(d, out): the table's bytes, or with `out` the table written there from
 * the entries' launches `d`, returning its runs; launch: its kernel. */
template <class OutOf, class Table, class Launch>
static int decompress_windows_of(Backend* b, const DecompressDeviceJob* entries, uint32_t entry_count, const std::vector<uint8_t>& used, uint32_t region_count,
                                 void* job_stream, const char* what, OutOf out_of, Table table, Launch launch, uint32_t buffers)
{
	return run_on_owner(b, entries[0].device_blocks, nullptr, 0, job_stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		auto foreign = [s](const void* p)
		{
			hipPointerAttribute_t attr;
			memset(&attr, 0, sizeof(attr));
			if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
			return attr.device != s->device;
		};
		for (uint32_t e = 0; e < entry_count; e++)
			if (used[e] && foreign(entries[e].device_blocks))
			{
				log_msg("%s: the blocks of entry %u are not on device %d, which owns entry 0's", what, e, s->device);
				return 3;
			}
		for (uint32_t i = 0; i < region_count * buffers; i++)
			if (foreign(out_of(i)))
			{
				log_msg("%s: the buffer of region %u is not on device %d, which owns entry 0's blocks", what, i / buffers, s->device);
				return 3;
			}
		std::vector<DecodeLaunch> d(entry_count);
		for (uint32_t e = 0; e < entry_count; e++) d[e] = decode_launch(b, s, entries[e], entries[e].device_blocks, nullptr, nullptr);
		const size_t bytes = table(d.data(), nullptr);
		s->h_set.assign(bytes, 0);
		const uint32_t runs = (uint32_t)table(d.data(), s->h_set.data());
		const int urc = set_table_upload(s, stream, bytes);
		if (urc != 0) return urc;
		int lrc = launch(s->d_set, runs, stream);
		if (lrc != 0) { log_msg("decode kernel launch failed (hip error %d)", lrc); return 2; }
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		return 0;
	});
}

/* (a region names one entry: used[e] of decompress_windows_of from entry_of) */
template <class EntryOf, class OutOf, class Table, class Launch>
static int decompress_windows(Backend* b, const DecompressDeviceJob* entries, uint32_t entry_count, uint32_t region_count, void* job_stream,
                              const char* what, EntryOf entry_of, OutOf out_of, Table table, Launch launch, uint32_t buffers = 1)
{
	std::vector<uint8_t> used(entry_count, 0);
	for (uint32_t i = 0; i < region_count; i++) used[entry_of(i)] = 1;
	return decompress_windows_of(b, entries, entry_count, used, region_count, job_stream, what, out_of, table, launch, buffers);
}

int backend_decompress_regions(Backend* b, const DecompressRegionsJob& job)
{
	return decompress_windows(b, job.entries, job.entry_count, job.region_count, job.stream, "decode regions",
		[&](uint32_t i) { return job.regions[i].entry; }, [&](uint32_t i) { return job.regions[i].d_out; },
		[&](const DecodeLaunch* d, void* out) -> size_t
		{
			return out ? astc_decode_regions_build(out, d, job.entry_count, job.regions, job.region_count) : astc_decode_regions_bytes(job.region_count);
		},
		astc_decode_regions_launch);
}

int backend_decompress_tensors(Backend* b, const DecompressTensorsJob& job)
{
	return decompress_windows(b, job.entries, job.entry_count, job.region_count, job.stream, "decode tensors",
		[&](uint32_t i) { return job.regions[i].entry; }, [&](uint32_t i) { return job.regions[i].d_out; },
		[&](const DecodeLaunch* d, void* out) -> size_t
		{
			return out ? astc_decode_tensors_build(out, d, job.entry_count, *job.format, job.regions, job.region_count) : astc_decode_tensors_bytes(job.region_count);
		},
		[&](const void* d_table, uint32_t runs, void* stream) { return astc_decode_tensors_launch(d_table, runs, job.format->type, job.format->layout, stream); });
}

int backend_decompress_scaled(Backend* b, const DecompressScaledJob& job)
{
	return decompress_windows(b, job.entries, job.entry_count, job.region_count, job.stream, "decode scaled tensors",
		[&](uint32_t i) { return job.regions[i].entry; }, [&](uint32_t i) { return job.regions[i].d_out; },
		[&](const DecodeLaunch* d, void* out) -> size_t
		{
			return out ? astc_decode_scaled_build(out, d, job.entry_count, *job.format, job.filter, job.regions, job.region_count) : astc_decode_scaled_bytes(job.region_count);
		},
		[&](const void* d_table, uint32_t tiles, void* stream) { return astc_decode_scaled_launch(d_table, tiles, job.format->type, job.format->layout, stream); });
}

/* (the coordinates are checked with the outputs: both are buffers of the grid) */
int backend_decompress_sample(Backend* b, const DecompressSampleJob& job)
{
	return decompress_windows(b, job.entries, job.entry_count, job.grid_count, job.stream, "sample tensors",
		[&](uint32_t i) { return job.grids[i].entry; },
		[&](uint32_t i) { return (i & 1u) ? static_cast<const void*>(job.grids[i >> 1].d_coords) : static_cast<const void*>(job.grids[i >> 1].d_out); },
		[&](const DecodeLaunch* d, void* out) -> size_t
		{
			return out ? astc_decode_sample_build(out, d, job.entry_count, *job.format, *job.sampler, job.grids, job.grid_count) : astc_decode_sample_bytes(job.grid_count);
		},
		[&](const void* d_table, uint32_t tiles, void* stream) { return astc_decode_sample_launch(d_table, tiles, job.format->type, job.format->layout, stream); }, 2u);
}

/* The level-of-detail samplers (the lod call, its gradient, the cube call, the volume call), `job` one of their jobs: a grid uses
 * the entries of all its levels; its buffers are the output (the gradient's grad_out), the points and the levels of detail -- the
 * output stands in for a null lod -- and the `extras` more that extra(grid, k) names.  bytes, build and launch: the call's table
 * and kernel (backend.h). */
template <class Job, class Grid>
static int decompress_lod_grids(Backend* b, const Job& job, const char* what, size_t (*bytes)(const Grid*, uint32_t),
                                uint32_t (*build)(void*, const DecodeLaunch*, uint32_t, const DecodeTensorFormat&, const DecodeLodSampler&, const Grid*, uint32_t),
                                int (*launch)(const void*, uint32_t, uint32_t, uint32_t, void*), uint32_t extras = 0, const void* (*extra)(const Grid&, uint32_t) = nullptr)
{
	std::vector<uint8_t> used(job.entry_count, 0);
	for (uint32_t i = 0; i < job.grid_count; i++)
	{
		const DecodeLodLaunch& g = decode_lod_launch_of(job.grids[i]);
		for (uint32_t l = 0; l < g.level_count; l++) used[g.first_entry + l] = 1;
	}
	const uint32_t buffers = 3u + extras;
	return decompress_windows_of(b, job.entries, job.entry_count, used, job.grid_count, job.stream, what,
		[&](uint32_t i) -> const void*
		{
			const DecodeLodLaunch& g = decode_lod_launch_of(job.grids[i / buffers]);
			const uint32_t k = i % buffers;
			return k == 0u || (k == 2u && !g.d_lod) ? g.d_out : k == 1u ? g.d_coords : k == 2u ? g.d_lod : extra(job.grids[i / buffers], k - 3u);
		},
		[&](const DecodeLaunch* d, void* out) -> size_t
		{
			return out ? build(out, d, job.entry_count, *job.format, *job.sampler, job.grids, job.grid_count) : bytes(job.grids, job.grid_count);
		},
		[&](const void* d_table, uint32_t tiles, void* stream) { return launch(d_table, tiles, job.format->type, job.format->layout, stream); }, buffers);
}

int backend_decompress_lod(Backend* b, const DecompressLodJob& job)
{
	return decompress_lod_grids(b, job, "sample lod tensors", astc_decode_lod_bytes, astc_decode_lod_build, astc_decode_lod_launch);
}

/* (the buffers that are written: grad_coords, and grad_lod, for which grad_coords stands in when it is null) */
static const void* lod_grad_buffer(const DecodeLodGradLaunch& g, uint32_t k)
{
	return k == 0u || !g.d_grad_lod ? g.d_grad_coords : g.d_grad_lod;
}

int backend_decompress_lod_grad(Backend* b, const DecompressLodGradJob& job)
{
	return decompress_lod_grids(b, job, "sample lod grad", astc_decode_lod_grad_bytes, astc_decode_lod_grad_build, astc_decode_lod_grad_launch, 2u, lod_grad_buffer);
}

int backend_decompress_cube(Backend* b, const DecompressLodJob& job)
{
	return decompress_lod_grids(b, job, "sample cube tensors", astc_decode_cube_bytes, astc_decode_cube_build, astc_decode_cube_launch);
}

int backend_decompress_volume(Backend* b, const DecompressLodJob& job)
{
	return decompress_lod_grids(b, job, "sample volume tensors", astc_decode_volume_bytes, astc_decode_volume_build, astc_decode_volume_launch);
}

int backend_decompress_volume_grad(Backend* b, const DecompressLodGradJob& job)
{
	return decompress_lod_grids(b, job, "sample volume grad", astc_decode_volume_grad_bytes, astc_decode_volume_grad_build, astc_decode_volume_grad_launch, 2u, lod_grad_buffer);
}

/* astcenc_amd_compare_blocks_device and its kin: the set's table is uploaded like the decoder's, the scratch for the partial
 * sums has a fixed size (rc 1 when it cannot be had, nothing launched), the totals come back once the stream has run. */
static int compare_blocks_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const QualitySetJob& job)
{
	std::vector<QualityLaunch> q(job.count);
	for (uint32_t e = 0; e < job.count; e++)
	{
		const QualityEntryJob& en = job.entries[e];
		hipPointerAttribute_t attr;
		memset(&attr, 0, sizeof(attr));
		if (en.device_block_errors && hipPointerGetAttributes(&attr, en.device_block_errors) == hipSuccess && attr.device != s->device)
		{
			log_msg("image set entry %u: the block error buffer is on device %d, entry 0's image on device %d", e, attr.device, s->device);
			return 3;
		}
		(void)hipGetLastError();
		q[e].decode = decode_launch(b, s, en.decode, en.decode.device_blocks, nullptr, nullptr);
		q[e].d_original = en.device_original; q[e].original_type = en.original_type;
		q[e].d_block_errors = en.device_block_errors;
	}
	const size_t sums_bytes = (size_t)job.count * METRIC_SUMS_HOST * sizeof(double);
	if (grow(s->d_quality, s->quality_cap, astc_quality_scratch_doubles() * sizeof(double)) != 0 ||
	    grow(s->d_quality_sums, s->quality_sums_cap, sums_bytes) != 0) return 1;
	const size_t bytes = astc_quality_set_bytes(job.count);
	s->h_set.assign(bytes, 0);
	astc_quality_set_build(s->h_set.data(), q.data(), job.count);
	// (a set of one entry -- the single-image calls -- needs no table on the device)
	const int urc = job.count > 1 ? set_table_upload(s, stream, bytes) : 0;
	if (urc != 0) return urc;
	int lrc = astc_quality_set_launch(s->h_set.data(), job.count > 1 ? s->d_set : nullptr, s->d_quality, s->d_quality_sums, job.hdr, job.fstop_lo, job.fstop_hi, stream);
	if (lrc != 0) { log_msg("block quality kernel launch failed (hip error %d)", lrc); return 2; }
	std::vector<double> raw((size_t)job.count * METRIC_SUMS_HOST);
	HIP_TRY(hipMemcpyAsync(raw.data(), s->d_quality_sums, sums_bytes, hipMemcpyDeviceToHost, stream), return 2);
	HIP_TRY(hipStreamSynchronize(stream), return 2);
	memcpy(job.sums, raw.data(), sums_bytes);
	return 0;
}

int backend_compare_blocks_set(Backend* b, const QualitySetJob& job)
{
	std::vector<const void*> ptrs;
	for (uint32_t e = 0; e < job.count; e++) { ptrs.push_back(job.entries[e].device_original); ptrs.push_back(job.entries[e].decode.device_blocks); }
	return run_on_owner(b, job.entries[0].device_original, ptrs.data(), ptrs.size(), job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		return compare_blocks_on_slot(b, s, stream, job);
	});
}

/* The selection launches of `job` on slot `s` (list: where the indices go); the count stays on the device, at *d_count. */
static int select_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const SelectJob& job, uint32_t* d_list, const uint32_t** d_count)
{
	const size_t blocks = job.blocks;
	// (one word past the counts: the merge kernel's counter)
	if (grow(s->d_select, s->select_cap, (astc_select_scratch_words(blocks) + 1) * sizeof(uint32_t)) != 0) return 1;
	SelectLaunch l;
	l.d_errors = job.device_block_errors;
	l.dim_x = job.dim_x; l.dim_y = job.dim_y; l.dim_z = job.dim_z;
	l.block_x = b->root.dim_x; l.block_y = b->root.dim_y; l.block_z = b->root.dim_z; l.blocks = job.blocks;
	for (int i = 0; i < 4; i++) l.weight[i] = job.weight[i];
	l.max_mse = job.max_mse;
	l.d_list = d_list; l.d_counts = s->d_select; l.stream = stream;
	const int lrc = astc_select_launch(l);
	if (lrc != 0) { log_msg("block selection kernel launch failed (hip error %d)", lrc); return 2; }
	*d_count = s->d_select + astc_select_total_word(blocks);
	return 0;
}

int backend_select_blocks(Backend* b, const SelectJob& job)
{
	const void* ptrs[1] = { job.device_list };
	return run_on_owner(b, job.device_block_errors, ptrs, 1, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		const uint32_t* d_count = nullptr;
		const int rc = select_on_slot(b, s, stream, job, job.device_list, &d_count);
		if (rc != 0) return rc;
		uint32_t count = 0;
		HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		*job.count = count;
		return 0;
	});
}

/* astcenc_amd_compress_image_adaptive_device after its base pass (job.strong.device_out holds the base stream B0), all of it on
 * the strong context's slot of the device that owns the image and on one stream:
 *   score B0 -> E0 (the caller's records, or scratch) | select E0 -> list, count | with no block selected, done
 *   copy B0 -> S (scratch) | strong pass over the list into S | score S -> E1 (scratch) | merge: S and E1 over B0 and E0 where better
 * Scratch: S, E1, E0 unless the caller's, the list: 16 + 32 (+ 32) + 4 bytes per block, sized before anything is launched. */
static size_t adaptive_scratch_bytes(size_t blocks, bool own_records) { return blocks * (16 + 32 + (own_records ? 32 : 0) + 4); }

int backend_adaptive_reserve(Backend* b, const void* device_image, const void* device_out, const void* device_block_errors, size_t blocks)
{
	const void* ptrs[2] = { device_out, device_block_errors };
	const bool own_records = device_block_errors == nullptr;
	return run_on_owner(b, device_image, ptrs, 2, nullptr, [&](DeviceSlot* s, hipStream_t)
	{
		if (grow(s->d_adaptive, s->adaptive_cap, adaptive_scratch_bytes(blocks, own_records)) != 0 ||
		    grow(s->d_select, s->select_cap, (astc_select_scratch_words(blocks) + 1) * sizeof(uint32_t)) != 0 ||
		    grow(s->d_quality, s->quality_cap, astc_quality_scratch_doubles() * sizeof(double)) != 0 ||
		    grow(s->d_quality_sums, s->quality_sums_cap, METRIC_SUMS_HOST * sizeof(double)) != 0) return 1;
		return 0;
	});
}

int backend_adaptive_refine(Backend* b, const AdaptiveJob& job)
{
	const CompressJob& cj = job.strong;
	const void* ptrs[2] = { cj.device_out, job.device_block_errors };
	return run_on_owner(b, cj.device_data, ptrs, 2, cj.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		const size_t blocks = block_grid(b->root, cj).count();
		const size_t at_e1 = blocks * 16, at_e0 = at_e1 + blocks * 32, at_list = at_e0 + (job.device_block_errors ? 0 : blocks * 32);
		if (grow(s->d_adaptive, s->adaptive_cap, adaptive_scratch_bytes(blocks, !job.device_block_errors)) != 0) return 1;
		uint8_t* d_stream = s->d_adaptive;
		double* d_e1 = reinterpret_cast<double*>(s->d_adaptive + at_e1);
		double* d_e0 = job.device_block_errors ? job.device_block_errors : reinterpret_cast<double*>(s->d_adaptive + at_e0);
		uint32_t* d_list = reinterpret_cast<uint32_t*>(s->d_adaptive + at_list);
		const bool timed = job.kernel_ms_other != nullptr;
		if (timed)
		{
			for (hipEvent_t& e : s->ev_adapt) if (!e) HIP_TRY(hipEventCreate(&e), return 2);
			HIP_TRY(hipEventRecord(s->ev_adapt[0], stream), return 2);
		}
		double sums[METRIC_SUMS_HOST];
		QualityEntryJob q;
		memset(&q, 0, sizeof(q));
		q.decode = job.decode;
		q.decode.device_blocks = cj.device_out;
		q.device_original = cj.device_data; q.original_type = cj.data_type;
		q.device_block_errors = d_e0;
		QualitySetJob qs;
		memset(&qs, 0, sizeof(qs));
		qs.entries = &q; qs.count = 1; qs.stream = stream; qs.sums = sums;
		int rc = compare_blocks_on_slot(b, s, stream, qs);
		if (rc != 0) return rc;

		SelectJob sj;
		memset(&sj, 0, sizeof(sj));
		sj.device_block_errors = d_e0;
		sj.dim_x = cj.dim_x; sj.dim_y = cj.dim_y; sj.dim_z = cj.dim_z ? cj.dim_z : 1u;
		sj.blocks = (uint32_t)blocks;
		for (int i = 0; i < 4; i++) sj.weight[i] = job.weight[i];
		sj.max_mse = job.max_mse;
		const uint32_t* d_count = nullptr;
		rc = select_on_slot(b, s, stream, sj, d_list, &d_count);
		if (rc != 0) return rc;
		uint32_t count = 0;
		HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		*job.selected = count;
		*job.replaced = 0;
		float strong_ms = 0.0f;
		if (count != 0)
		{
			HIP_TRY(hipMemcpyAsync(d_stream, cj.device_out, blocks * 16, hipMemcpyDeviceToDevice, stream), return 2);
			CompressJob lj = cj;
			lj.device_out = d_stream;
			lj.device_list = d_list; lj.list_count = count;
			lj.kernel_ms = timed ? &strong_ms : nullptr;
			Progress progress;
			progress.done = 0; progress.callback = lj.progress; progress.total = count;
			rc = compress_on_slot(b, s, stream, lj, &progress);
			if (rc != 0) return rc;
			q.decode.device_blocks = d_stream;
			q.device_block_errors = d_e1;
			rc = compare_blocks_on_slot(b, s, stream, qs);
			if (rc != 0) return rc;
			uint32_t* d_replaced = s->d_select + astc_select_scratch_words(blocks);
			MergeLaunch m;
			m.d_list = d_list; m.d_count = d_count; m.blocks = (uint32_t)blocks; m.max_count = count;
			m.d_strong_errors = d_e1; m.d_base_errors = d_e0;
			m.d_strong = d_stream; m.d_out = cj.device_out;
			for (int i = 0; i < 4; i++) m.weight[i] = job.weight[i];
			m.d_replaced = d_replaced; m.stream = stream;
			const int mrc = astc_merge_launch(m);
			if (mrc != 0) { log_msg("block merge kernel launch failed (hip error %d)", mrc); return 2; }
			HIP_TRY(hipMemcpyAsync(job.replaced, d_replaced, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), return 2);
		}
		if (timed) HIP_TRY(hipEventRecord(s->ev_adapt[1], stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		if (timed)
		{
			float all_ms = 0.0f;
			HIP_TRY(hipEventElapsedTime(&all_ms, s->ev_adapt[0], s->ev_adapt[1]), return 2);
			*job.kernel_ms_strong = strong_ms;
			*job.kernel_ms_other = all_ms > strong_ms ? all_ms - strong_ms : 0.0f;
		}
		return 0;
	});
}

/* The selection launches of `job` over its set on slot `s` (d_list: where the indices go).  The candidate count and the list's
 * length stay on the device, at astc_budget_counts(s->d_budget_fixed); the table stays at s->d_budget_tab for the merge. */
static int select_set_on_slot(Backend* b, DeviceSlot* s, hipStream_t stream, const SelectSetJob& job, uint32_t* d_list)
{
	const size_t blocks = job.blocks;
	const size_t table_bytes = astc_budget_table_bytes(job.count);
	// (one word past the counts: the merge kernel's counter)
	if (grow(s->d_select, s->select_cap, (astc_budget_count_words(blocks) + 1) * sizeof(uint32_t)) != 0 ||
	    grow(s->d_keys, s->keys_cap, blocks * sizeof(unsigned long long)) != 0 ||
	    grow(s->d_budget_fixed, s->budget_fixed_cap, astc_budget_fixed_bytes()) != 0 ||
	    grow(s->d_budget_tab, s->budget_tab_cap, table_bytes) != 0) return 1;
	s->h_budget_tab.assign(table_bytes, 0);
	astc_budget_table_build(s->h_budget_tab.data(), job.entries, job.count, b->root.dim_x, b->root.dim_y, b->root.dim_z);
	HIP_TRY(hipMemcpyAsync(s->d_budget_tab, s->h_budget_tab.data(), table_bytes, hipMemcpyHostToDevice, stream), return 2);
	BudgetSelectLaunch l;
	l.d_errors = job.device_block_errors; l.d_table = s->d_budget_tab;
	l.block_x = b->root.dim_x; l.block_y = b->root.dim_y; l.block_z = b->root.dim_z; l.blocks = job.blocks;
	for (int i = 0; i < 4; i++) l.weight[i] = job.weight[i];
	l.max_mse = job.max_mse; l.max_blocks = job.max_blocks;
	l.d_keys = s->d_keys; l.d_counts = s->d_select; l.d_fixed = s->d_budget_fixed; l.d_list = d_list; l.stream = stream;
	const int lrc = astc_budget_select_launch(l);
	if (lrc != 0) { log_msg("block selection kernel launch failed (hip error %d)", lrc); return 2; }
	return 0;
}

int backend_select_blocks_set(Backend* b, const SelectSetJob& job)
{
	const void* ptrs[1] = { job.device_list };
	return run_on_owner(b, job.device_block_errors, ptrs, 1, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		const int rc = select_set_on_slot(b, s, stream, job, job.device_list);
		if (rc != 0) return rc;
		uint32_t counts[2] = { 0, 0 };
		HIP_TRY(hipMemcpyAsync(counts, astc_budget_counts(s->d_budget_fixed), sizeof(counts), hipMemcpyDeviceToHost, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		if (job.candidates) *job.candidates = counts[0];
		*job.selected = counts[1];
		return 0;
	});
}

/* astcenc_amd_compress_images_adaptive_device after its base pass: backend_adaptive_refine over a set.  The strong stream S and the
 * records E0, E1 are laid out by the global block index, entry after entry; the strong pass is a block-list launch of the set
 * whose entries write into their parts of S, and the merge stores into the entries' own buffers through the selection's table.
 * Scratch: S, E1, E0 unless the caller's, the list, the keys: 16 + 32 (+ 32) + 4 + 8 bytes per block, sized before anything is
 * launched. */
static size_t set_blocks(const Backend* b, const CompressSetJob& set, std::vector<size_t>* first)
{
	size_t total = 0;
	for (uint32_t e = 0; e < set.count; e++)
	{
		if (first) first->push_back(total);
		total += block_grid(b->root, set.entries[e]).count();
	}
	return total;
}

static std::vector<const void*> set_pointers(const CompressSetJob& set, const void* device_block_errors)
{
	std::vector<const void*> ptrs;
	for (uint32_t e = 0; e < set.count; e++) { ptrs.push_back(set.entries[e].device_data); ptrs.push_back(set.entries[e].device_out); }
	ptrs.push_back(device_block_errors); ptrs.push_back(nullptr);
	return ptrs;
}

int backend_adaptive_set_reserve(Backend* b, const CompressSetJob& set, const void* device_block_errors, size_t blocks)
{
	const std::vector<const void*> ptrs = set_pointers(set, device_block_errors);
	const bool own_records = device_block_errors == nullptr;
	return run_on_owner(b, set.entries[0].device_data, ptrs.data(), ptrs.size(), nullptr, [&](DeviceSlot* s, hipStream_t)
	{
		if (grow(s->d_adaptive, s->adaptive_cap, adaptive_scratch_bytes(blocks, own_records)) != 0 ||
		    grow(s->d_select, s->select_cap, (astc_budget_count_words(blocks) + 1) * sizeof(uint32_t)) != 0 ||
		    grow(s->d_keys, s->keys_cap, blocks * sizeof(unsigned long long)) != 0 ||
		    grow(s->d_budget_fixed, s->budget_fixed_cap, astc_budget_fixed_bytes()) != 0 ||
		    grow(s->d_budget_tab, s->budget_tab_cap, astc_budget_table_bytes(set.count)) != 0 ||
		    grow(s->d_quality, s->quality_cap, astc_quality_scratch_doubles() * sizeof(double)) != 0 ||
		    grow(s->d_quality_sums, s->quality_sums_cap, (size_t)set.count * METRIC_SUMS_HOST * sizeof(double)) != 0) return 1;
		return 0;
	});
}

int backend_adaptive_set_refine(Backend* b, const AdaptiveSetJob& job)
{
	const CompressSetJob& cs = job.strong;
	const std::vector<const void*> ptrs = set_pointers(cs, job.device_block_errors);
	return run_on_owner(b, cs.entries[0].device_data, ptrs.data(), ptrs.size(), cs.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		std::vector<size_t> first;
		const size_t blocks = set_blocks(b, cs, &first);
		const size_t at_e1 = blocks * 16, at_e0 = at_e1 + blocks * 32, at_list = at_e0 + (job.device_block_errors ? 0 : blocks * 32);
		if (grow(s->d_adaptive, s->adaptive_cap, adaptive_scratch_bytes(blocks, !job.device_block_errors)) != 0) return 1;
		uint8_t* d_stream = s->d_adaptive;
		double* d_e1 = reinterpret_cast<double*>(s->d_adaptive + at_e1);
		double* d_e0 = job.device_block_errors ? job.device_block_errors : reinterpret_cast<double*>(s->d_adaptive + at_e0);
		uint32_t* d_list = reinterpret_cast<uint32_t*>(s->d_adaptive + at_list);
		const bool timed = job.kernel_ms_other != nullptr;
		if (timed)
		{
			for (hipEvent_t& e : s->ev_adapt) if (!e) HIP_TRY(hipEventCreate(&e), return 2);
			HIP_TRY(hipEventRecord(s->ev_adapt[0], stream), return 2);
		}
		std::vector<double> sums((size_t)cs.count * METRIC_SUMS_HOST);
		std::vector<QualityEntryJob> q(job.score, job.score + cs.count);
		for (uint32_t e = 0; e < cs.count; e++) q[e].device_block_errors = d_e0 + first[e] * 4;
		QualitySetJob qs;
		memset(&qs, 0, sizeof(qs));
		qs.entries = q.data(); qs.count = cs.count; qs.stream = stream; qs.sums = sums.data();
		int rc = compare_blocks_on_slot(b, s, stream, qs);
		if (rc != 0) return rc;

		std::vector<BudgetSetEntry> dims(cs.count);
		for (uint32_t e = 0; e < cs.count; e++)
			dims[e] = { cs.entries[e].dim_x, cs.entries[e].dim_y, cs.entries[e].dim_z ? cs.entries[e].dim_z : 1u, cs.entries[e].device_out };
		SelectSetJob sj;
		memset(&sj, 0, sizeof(sj));
		sj.device_block_errors = d_e0;
		sj.entries = dims.data(); sj.count = cs.count; sj.blocks = (uint32_t)blocks;
		for (int i = 0; i < 4; i++) sj.weight[i] = job.weight[i];
		sj.max_mse = job.max_mse; sj.max_blocks = job.max_blocks;
		rc = select_set_on_slot(b, s, stream, sj, d_list);
		if (rc != 0) return rc;
		uint32_t counts[2] = { 0, 0 };
		HIP_TRY(hipMemcpyAsync(counts, astc_budget_counts(s->d_budget_fixed), sizeof(counts), hipMemcpyDeviceToHost, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		*job.candidates = counts[0];
		*job.selected = counts[1];
		*job.replaced = 0;
		const uint32_t count = counts[1];
		float strong_ms = 0.0f;
		if (count != 0)
		{
			std::vector<CompressJob> entries(cs.entries, cs.entries + cs.count);
			for (uint32_t e = 0; e < cs.count; e++)
			{
				const size_t bytes = (e + 1 < cs.count ? first[e + 1] - first[e] : blocks - first[e]) * 16;
				HIP_TRY(hipMemcpyAsync(d_stream + first[e] * 16, cs.entries[e].device_out, bytes, hipMemcpyDeviceToDevice, stream), return 2);
				entries[e].device_out = d_stream + first[e] * 16;
			}
			CompressSetJob lj = cs;
			lj.entries = entries.data();
			lj.device_list = d_list; lj.list_count = count;
			lj.kernel_ms = timed ? &strong_ms : nullptr;
			lj.generate = nullptr;
			Progress progress;
			progress.done = 0; progress.callback = lj.progress; progress.total = count;
			rc = compress_set_on_slot(b, s, stream, lj, &progress);
			if (rc != 0) return rc;
			for (uint32_t e = 0; e < cs.count; e++)
			{
				q[e].decode.device_blocks = d_stream + first[e] * 16;
				q[e].device_block_errors = d_e1 + first[e] * 4;
			}
			rc = compare_blocks_on_slot(b, s, stream, qs);
			if (rc != 0) return rc;
			uint32_t* d_replaced = s->d_select + astc_budget_count_words(blocks);
			MergeSetLaunch m;
			m.d_list = d_list; m.d_fixed = s->d_budget_fixed; m.max_count = count;
			m.d_strong_errors = d_e1; m.d_base_errors = d_e0;
			m.d_strong = d_stream; m.d_table = s->d_budget_tab;
			for (int i = 0; i < 4; i++) m.weight[i] = job.weight[i];
			m.d_replaced = d_replaced; m.stream = stream;
			const int mrc = astc_merge_set_launch(m);
			if (mrc != 0) { log_msg("block merge kernel launch failed (hip error %d)", mrc); return 2; }
			HIP_TRY(hipMemcpyAsync(job.replaced, d_replaced, sizeof(uint32_t), hipMemcpyDeviceToHost, stream), return 2);
		}
		if (timed) HIP_TRY(hipEventRecord(s->ev_adapt[1], stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		if (timed)
		{
			float all_ms = 0.0f;
			HIP_TRY(hipEventElapsedTime(&all_ms, s->ev_adapt[0], s->ev_adapt[1]), return 2);
			*job.kernel_ms_strong = strong_ms;
			*job.kernel_ms_other = all_ms > strong_ms ? all_ms - strong_ms : 0.0f;
		}
		return 0;
	});
}

int backend_generate_mips(Backend* b, const MipChainJob& job)
{
	// (the device check of a set: the image and the levels buffer -- the one allocation every generated level lies in)
	const void* ptrs[2] = { job.device_image, job.level_count > 1 ? job.device_levels : nullptr };
	return run_on_owner(b, job.device_image, ptrs, 2, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		const int grc = generate_mips_locked(s, stream, job);
		if (grc != 0) return grc;
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		return 0;
	});
}

/* astcenc_amd_resize_image_device: the taps are sized and built first (rc 1 when they exceed the scratch bound, nothing
 * launched), uploaded into the slot's mip filter scratch and the kernel queued behind them; kernel_ms is the kernel's. */
int backend_resize(Backend* b, const ResizeJob& job)
{
	const void* ptrs[2] = { job.device_image, job.device_out };
	return run_on_owner(b, job.device_image, ptrs, 2, job.stream, [&](DeviceSlot* s, hipStream_t stream)
	{
		if (astc_resize_table_build(job, s->h_mip_filter) != 0) { log_msg("resize: the taps exceed the 64 MiB scratch bound"); return 1; }
		const size_t bytes = s->h_mip_filter.size();
		if (grow(s->d_mip_filter, s->mip_filter_cap, bytes) != 0) return 1;
		HIP_TRY(hipMemcpyAsync(s->d_mip_filter, s->h_mip_filter.data(), bytes, hipMemcpyHostToDevice, stream), return 2);
		if (job.kernel_ms) HIP_TRY(hipEventRecord(s->ev0, stream), return 2);
		const int lrc = astc_resize_launch(job, s->d_mip_filter, s->d_srgb, stream);
		if (lrc != 0) { log_msg("resize kernel launch failed (hip error %d)", lrc); return 2; }
		if (job.kernel_ms) HIP_TRY(hipEventRecord(s->ev1, stream), return 2);
		HIP_TRY(hipStreamSynchronize(stream), return 2);
		if (job.kernel_ms) HIP_TRY(hipEventElapsedTime(job.kernel_ms, s->ev0, s->ev1), return 2);
		return 0;
	});
}

} // namespace astcd
