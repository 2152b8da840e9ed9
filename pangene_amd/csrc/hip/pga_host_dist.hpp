// pga_pan_shared (include/pangene_hip.h): the shared-item matrix of pangene dist on the device (k_dist.hpp).  Context-free: it runs
// on a stream of its own on the current device.  The device buffers and the page-locked result are kept from call to call and only
// ever grow; pga_host_trim(0) gives them back.  The result waits in the page-locked buffer until the next call.

constexpr int32_t DIST_MAX_ASM = 65535;

namespace {
struct DistDev {
	std::mutex mu;
	hipStream_t st = nullptr;
	enum { BITS, OUT, N_BUF };
	void *p[N_BUF] = {};
	size_t cap[N_BUF] = {};
	int32_t *host = nullptr; // page-locked result
	size_t host_cap = 0;
	template <class T> T *get(int i, size_t n) // at least n elements of T in buffer i (contents not kept)
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
	int32_t *get_host(size_t n)
	{
		const size_t bytes = sizeof(int32_t) * (n ? n : 1);
		if (host_cap < bytes) {
			if (host) (void)hipHostFree(host);
			host = nullptr, host_cap = 0;
			if (hipHostMalloc((void **)&host, bytes, hipHostMallocDefault) != hipSuccess) { host = nullptr; return nullptr; }
			host_cap = bytes;
		}
		return host;
	}
	void release()
	{
		for (int i = 0; i < N_BUF; ++i) { if (p[i]) (void)hipFree(p[i]); p[i] = nullptr, cap[i] = 0; }
		if (host) (void)hipHostFree(host);
		host = nullptr, host_cap = 0;
	}
};
DistDev g_dist;
}

static void dist_release() { std::lock_guard<std::mutex> lk(g_dist.mu); g_dist.release(); }

#define DISTCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::pga_pan_shared] %s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return PGA_ERR_NO_DEVICE; } } while (0)
#define DISTMEM(p) do { if ((p) == nullptr) return PGA_ERR_NOMEM; } while (0)

extern "C" int pga_pan_shared(const pga_shared_in_t *in, pga_shared_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->shared = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t M = in->n_item, A = in->n_asm;
	if (M < 0 || A < 0) return PGA_ERR_ARG;
	if (A > DIST_MAX_ASM) return PGA_ERR_RANGE;
	const int32_t W = (int32_t)(((int64_t)M + 31) / 32);
	if (A > 0 && W > 0 && in->bits == nullptr) return PGA_ERR_ARG;
	std::lock_guard<std::mutex> lk(g_dist.mu);
	DistDev &m = g_dist;
	const size_t nn = (size_t)A * (size_t)A;
	int32_t *h_out = m.get_host(nn);
	DISTMEM(h_out);
	out->shared = h_out;
	if (A == 0) return 0;
	if (W == 0) { memset(h_out, 0, sizeof(int32_t) * nn); return 0; }
	const int32_t n_chunk = (W + DIST_KC - 1) / DIST_KC, T = (A + DIST_TILE - 1) / DIST_TILE, n_tile = T * (T + 1) / 2;
	// fewer tiles than two workgroups per CU on 256 CUs: the tiles' K chunks are split over several workgroups that add into S
	const int32_t want = 512;
	int32_t n_split = n_tile >= want ? 1 : std::min(n_chunk, (want + n_tile - 1) / n_tile);
	const int32_t cps = (n_chunk + n_split - 1) / n_split;
	n_split = (n_chunk + cps - 1) / cps; // no empty slice
	if (m.st == nullptr) DISTCHK(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking));
	hipStream_t st = m.st;
	uint32_t *d_bits = m.get<uint32_t>(DistDev::BITS, (size_t)A * (size_t)W);
	int32_t *d_out = m.get<int32_t>(DistDev::OUT, nn);
	DISTMEM(d_bits); DISTMEM(d_out);
	DISTCHK(hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * (size_t)A * (size_t)W, hipMemcpyHostToDevice, st));
	if (n_split > 1) DISTCHK(hipMemsetAsync(d_out, 0, sizeof(int32_t) * nn, st));
	hipLaunchKernelGGL(k_dist_shared, dim3((unsigned)n_tile * (unsigned)n_split), dim3(BLOCK), 0, st, d_bits, A, W, n_chunk, n_split, cps, d_out);
	DISTCHK(hipGetLastError());
	DISTCHK(hipMemcpyAsync(h_out, d_out, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, st));
	DISTCHK(hipStreamSynchronize(st));
	return 0;
}
#undef DISTCHK
#undef DISTMEM
