// pga_host_pan.hpp -- the device state the context-free pga_pan_* entries keep from call to call: one pool per entry, each with a
// lock, a stream of its own on the current device, device buffers and page-locked host buffers.  The buffers only ever grow, and
// their contents are not kept across a growth; results a call leaves in a page-locked buffer stay valid until the same entry's next
// call.  Every entry locks its own pool, so two different entries may run at the same time.  pga_host_trim(0) gives all of it back
// (pan_release_all), and the next call allocates again.  Included by pga_backend.hip before the entries' headers; each of those keeps
// only its enum of buffer numbers.
#pragma once

constexpr int PAN_MAX_DEV = 16, PAN_MAX_HOST = 3; // buffers a pool has room for

enum PanEntry { PAN_CURVES, PAN_DIST, PAN_ASSOC, PAN_TRAIT, PAN_JOIN, PAN_BOOT, PAN_PAIRS, PAN_QTRAIT, PAN_MEDOIDS, PAN_PERMANOVA, PAN_MANTEL, PAN_N_ENTRY };

namespace {
struct PanDev {
	const char *name; // the entry, for error lines
	std::mutex mu;
	hipStream_t st = nullptr;
	void *p[PAN_MAX_DEV] = {};
	size_t cap[PAN_MAX_DEV] = {};
	void *host[PAN_MAX_HOST] = {}; // page-locked
	size_t host_cap[PAN_MAX_HOST] = {};
	PanDev(const char *n) : name(n) {}
	hipError_t stream(hipStream_t *out) // non-blocking, created at the first use
	{
		const hipError_t e = st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
		*out = st;
		return e;
	}
	template <class T> T *get(int i, size_t n) // at least n elements of T in device buffer i (contents not kept)
	{
		const size_t bytes = sizeof(T) * (n ? n : 1);
		if (cap[i] < bytes) {
			if (p[i]) (void)hipFree(p[i]);
			p[i] = nullptr, cap[i] = 0;
			if (hipMalloc(&p[i], bytes) != hipSuccess) { p[i] = nullptr; return nullptr; }
			cap[i] = bytes;
		}
		return (T *)p[i];
	}
	template <class T> T *get_host(int i, size_t n) // the same of page-locked buffer i
	{
		const size_t bytes = sizeof(T) * (n ? n : 1);
		if (host_cap[i] < bytes) {
			if (host[i]) (void)hipHostFree(host[i]);
			host[i] = nullptr, host_cap[i] = 0;
			if (hipHostMalloc(&host[i], bytes, hipHostMallocDefault) != hipSuccess) { host[i] = nullptr; return nullptr; }
			host_cap[i] = bytes;
		}
		return (T *)host[i];
	}
	void release()
	{
		for (int i = 0; i < PAN_MAX_DEV; ++i) { if (p[i]) (void)hipFree(p[i]); p[i] = nullptr, cap[i] = 0; }
		for (int i = 0; i < PAN_MAX_HOST; ++i) { if (host[i]) (void)hipHostFree(host[i]); host[i] = nullptr, host_cap[i] = 0; }
	}
};
PanDev g_pan[PAN_N_ENTRY] = {{"pga_pan_curves"}, {"pga_pan_shared"}, {"pga_pan_assoc"}, {"pga_pan_trait"}, {"pga_pan_join"}, {"pga_pan_boot"}, {"pga_pan_pairs"},
                            {"pga_pan_qtrait"}, {"pga_pan_medoids"}, {"pga_pan_permanova"}, {"pga_pan_mantel"}};
}

static void pan_release_all()
{
	for (PanDev &m : g_pan) { std::lock_guard<std::mutex> lk(m.mu); m.release(); }
}

// m: the entry's pool.  The lines read [E::pga_pan_xxx] file:line: message.
#define PANCHK(m, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::%s] %s:%d: %s\n", (m).name, __FILE__, __LINE__, hipGetErrorString(e_)); return PGA_ERR_NO_DEVICE; } } while (0)
#define PANMEM(p) do { if ((p) == nullptr) return PGA_ERR_NOMEM; } while (0)

// The split-K launch shape of k_dist_shared over A rows of W words: n_tile upper-triangle tiles, and where those are fewer than two
// workgroups per CU on 256 CUs, each tile's n_chunk K chunks in n_split slices of cps chunks (no empty slice) that add into S.
// W == 0 gives one slice of one (empty) chunk.
struct DistShape { int32_t n_chunk, n_tile, n_split, cps; };
static DistShape dist_shape(int32_t A, int32_t W)
{
	DistShape s;
	const int32_t T = (A + DIST_TILE - 1) / DIST_TILE, want = 512;
	s.n_chunk = (W + DIST_KC - 1) / DIST_KC, s.n_tile = T * (T + 1) / 2;
	const int32_t nc = std::max(s.n_chunk, 1);
	s.n_split = s.n_tile >= want ? 1 : std::min(nc, (want + s.n_tile - 1) / s.n_tile);
	s.cps = (nc + s.n_split - 1) / s.n_split;
	s.n_split = (nc + s.cps - 1) / s.cps;
	return s;
}
