// pga_host_pan.hpp -- the device state the context-free pga_pan_* entries keep from call to call: one pool per entry, each with a
// lock, a stream of its own on the current device, device buffers and page-locked host buffers.  The buffers only ever grow, and
// their contents are not kept across a growth; results a call leaves in a page-locked buffer stay valid until the same entry's next
// call.  Every entry locks its own pool, so two different entries may run at the same time.  pga_host_trim(0) gives all of it back
// (pan_release_all), and the next call allocates again.  Included by pga_backend.hip before the entries' headers; each of those keeps
// only its enum of buffer numbers.  Below the pools: the count switches (pan_env) and the batch driver of the permutation entries.
#pragma once

constexpr int PAN_MAX_DEV = 22, PAN_MAX_HOST = 3; // buffers a pool has room for

enum PanEntry { PAN_CURVES, PAN_DIST, PAN_ASSOC, PAN_TRAIT, PAN_JOIN, PAN_BOOT, PAN_PAIRS, PAN_QTRAIT, PAN_MEDOIDS, PAN_PERMANOVA, PAN_MANTEL, PAN_GAINLOSS, PAN_COEVO, PAN_PHYLOSIG, PAN_PCOA, PAN_GLM, PAN_RATES, PAN_N_ENTRY };

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
                            {"pga_pan_qtrait"}, {"pga_pan_medoids"}, {"pga_pan_permanova"}, {"pga_pan_mantel"}, {"pga_pan_gainloss"}, {"pga_pan_coevo"}, {"pga_pan_phylosig"}, {"pga_pan_pcoa"}, {"pga_pan_glm"}, {"pga_pan_rates"}};
}

static void pan_release_all()
{
	for (PanDev &m : g_pan) { std::lock_guard<std::mutex> lk(m.mu); m.release(); }
}

// m: the entry's pool.  The lines read [E::pga_pan_xxx] file:line: message.
#define PANCHK(m, x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::%s] %s:%d: %s\n", (m).name, __FILE__, __LINE__, hipGetErrorString(e_)); return PGA_ERR_NO_DEVICE; } } while (0)
#define PANMEM(p) do { if ((p) == nullptr) return PGA_ERR_NOMEM; } while (0)

// a switch NAME=v that takes a count, 1 <= v <= max; absent or anything else: def
static int64_t pan_env(const char *name, int64_t def, int64_t max)
{
	if (const char *s = getenv(name)) { const long long v = atoll(s); if (v >= 1 && v <= max) return v; }
	return def;
}

// The batch driver of the permutation entries (trait, qtrait, permanova, mantel, phylosig).  n permutations go through in batches of
// B = min(batch, max(n, 1)) rows made by a one-wave kernel of k_perm.hpp, whose 64 rows per workgroup live in LDS (lds) or in a scratch
// buffer of work(elems) elements:  for (PermBatches b(n, batch, lds); b.more(); b.next()) with b.p0(), b.nb(), b.first().
constexpr int32_t PAN_MAX_PERM = 2147483646; // 2^31 - 2

struct PermBatches {
	int32_t n, B;
	bool lds;
	int64_t done = 0;
	PermBatches(int32_t n_perm, int32_t batch, bool lds_) : n(n_perm), B((int32_t)std::min<int64_t>(batch, std::max<int32_t>(n_perm, 1))), lds(lds_) {}
	size_t work(size_t elems) const { return lds ? 1 : (size_t)(((int64_t)B + WAVE - 1) / WAVE) * elems * WAVE; }
	bool more() const { return done < n; }
	void next() { done += B; }
	uint32_t p0() const { return (uint32_t)(done + 1); } // permutations are numbered from 1
	int32_t nb() const { return (int32_t)std::min<int64_t>(B, (int64_t)n - done); }
	bool first() const { return done == 0; }
};

// the <true> (LDS) / <false> (scratch buffer) pair of a one-wave permutation kernel over the nb rows of a batch
template <class... P, class... A> static void perm_launch(bool lds, void (*k_lds)(P...), void (*k_work)(P...), int32_t nb, hipStream_t st, A... a)
{
	hipLaunchKernelGGL(lds ? k_lds : k_work, dim3((unsigned)((nb + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, (P)a...);
}

// the end of trait and qtrait: three device arrays of G counts into the planes h[0 .. 3 G), and the call's one wait
static int pan_download3(PanDev &m, hipStream_t st, int32_t *h, const int32_t *d0, const int32_t *d1, const int32_t *d2, int32_t G)
{
	const int32_t *d[3] = {d0, d1, d2};
	for (int i = 0; i < 3 && G > 0; ++i) PANCHK(m, hipMemcpyAsync(h + (size_t)i * (size_t)G, d[i], sizeof(int32_t) * (size_t)G, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}

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
