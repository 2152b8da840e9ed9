// pga_pan_curves (include/pangene_hip.h): accumulation curves on the device (k_curves.hpp).  Context-free: it runs on a stream of
// its own on the current device.  The device buffers are kept from call to call and only ever grow (a hipMalloc per call would cost
// more than the kernels); pga_host_trim(0) gives them back.  The result waits in a host vector of the library until the next call.

namespace {
struct CurvesDev {
	std::mutex mu;
	hipStream_t st = nullptr;
	enum { BITS, ORD, RANK, CNT, LEN, OFF, LIST, TILES, HIST, OUT, N_BUF };
	void *p[N_BUF] = {};
	size_t cap[N_BUF] = {};
	std::vector<int32_t> out;
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
	void release() { for (int i = 0; i < N_BUF; ++i) { if (p[i]) (void)hipFree(p[i]); p[i] = nullptr, cap[i] = 0; } }
};
CurvesDev g_curves;
}

static void curves_release() { std::lock_guard<std::mutex> lk(g_curves.mu); g_curves.release(); }

#define CURVCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::pga_pan_curves] %s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return PGA_ERR_NO_DEVICE; } } while (0)
#define CURVMEM(p) do { if ((p) == nullptr) return PGA_ERR_NOMEM; } while (0)

extern "C" int pga_pan_curves(const pga_curves_in_t *in, pga_curves_out_t *out)
{
	out->count = nullptr;
	const int32_t G = in->n_gene, A = in->n_asm, n = in->n_perm;
	if (G < 0 || A < 0 || n < 0) return PGA_ERR_ARG;
	{ // every order a permutation of the columns: the kernels index with them
		std::vector<uint8_t> seen((size_t)A);
		for (int32_t p = 0; p < n; ++p) {
			std::fill(seen.begin(), seen.end(), 0);
			const int32_t *o = in->order + (size_t)p * A;
			for (int32_t i = 0; i < A; ++i) { if (o[i] < 0 || o[i] >= A || seen[(size_t)o[i]]) return PGA_ERR_ARG; seen[(size_t)o[i]] = 1; }
		}
	}
	std::lock_guard<std::mutex> lk(g_curves.mu);
	CurvesDev &m = g_curves;
	m.out.assign((size_t)4 * n * A, 0);
	out->count = m.out.data();
	if (G == 0 || A == 0 || n == 0) return 0;
	const int32_t W = (A + 31) / 32;
	int32_t T = 2;
	while ((int64_t)T * T < 2 * (int64_t)A) ++T; // ceil(sqrt(2A))
	const int64_t list_max = (int64_t)G * std::min(T, A);
	if (list_max >= INT32_MAX || (int64_t)n * 3 * (A + 1) >= INT32_MAX || (int64_t)n * A >= INT32_MAX / 4) return PGA_ERR_RANGE;
	if (m.st == nullptr) CURVCHK(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking));
	hipStream_t st = m.st;
	uint32_t *d_bits = m.get<uint32_t>(CurvesDev::BITS, (size_t)G * W);
	int32_t *d_ord = m.get<int32_t>(CurvesDev::ORD, (size_t)n * A), *d_rank = m.get<int32_t>(CurvesDev::RANK, (size_t)n * A);
	int32_t *d_cnt = m.get<int32_t>(CurvesDev::CNT, (size_t)G), *d_len = m.get<int32_t>(CurvesDev::LEN, (size_t)G), *d_off = m.get<int32_t>(CurvesDev::OFF, (size_t)G);
	int32_t *d_list = m.get<int32_t>(CurvesDev::LIST, (size_t)list_max);
	I32 *d_tiles = m.get<I32>(CurvesDev::TILES, (size_t)scan_tiles(G));
	int32_t *d_hist = m.get<int32_t>(CurvesDev::HIST, (size_t)n * 3 * (A + 1)), *d_out = m.get<int32_t>(CurvesDev::OUT, (size_t)4 * n * A);
	CURVMEM(d_bits); CURVMEM(d_ord); CURVMEM(d_rank); CURVMEM(d_cnt); CURVMEM(d_len); CURVMEM(d_off); CURVMEM(d_list); CURVMEM(d_tiles); CURVMEM(d_hist); CURVMEM(d_out);
	CURVCHK(hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * (size_t)G * W, hipMemcpyHostToDevice, st));
	CURVCHK(hipMemcpyAsync(d_ord, in->order, sizeof(int32_t) * (size_t)n * A, hipMemcpyHostToDevice, st));
	CURVCHK(hipMemsetAsync(d_hist, 0, sizeof(int32_t) * (size_t)n * 3 * (A + 1), st));
	auto grid = [](int64_t k) { return dim3((unsigned)((k + BLOCK - 1) / BLOCK)); };
	hipLaunchKernelGGL(k_curves_rank, grid((int64_t)n * A), dim3(BLOCK), 0, st, d_ord, (int64_t)n * A, A, d_rank);
	hipLaunchKernelGGL(k_curves_count, grid(G), dim3(BLOCK), 0, st, d_bits, W, G, A, T, d_cnt, d_len);
	device_scan<I32>(InI32{d_len}, OutExclI32{d_off}, G, d_tiles, OpSum{}, I32{0}, st);
	hipLaunchKernelGGL(k_curves_fill, grid(G), dim3(BLOCK), 0, st, d_bits, W, G, A, T, d_cnt, d_off, d_list);
	// blocks per order: enough blocks in all to fill the device, never fewer than BLOCK genes per block
	const int32_t R = std::min(A, CURVES_LDS_BINS - 1);
	const int32_t bpo = (int32_t)std::max<int64_t>(1, std::min<int64_t>((G + BLOCK - 1) / BLOCK, (2048 + n - 1) / n));
	if ((int64_t)n * bpo >= INT32_MAX) return PGA_ERR_RANGE;
	hipLaunchKernelGGL(k_curves_ranks, dim3((unsigned)(n * bpo)), dim3(BLOCK), sizeof(int32_t) * 3 * (size_t)(R + 1), st, d_bits, W, d_ord, d_rank,
	                   d_cnt, d_off, d_list, G, A, T, R, bpo, d_hist);
	hipLaunchKernelGGL(k_curves_finish, dim3((unsigned)n), dim3(BLOCK), 0, st, d_hist, A, G, n, d_out);
	CURVCHK(hipGetLastError());
	CURVCHK(hipMemcpyAsync(m.out.data(), d_out, sizeof(int32_t) * m.out.size(), hipMemcpyDeviceToHost, st));
	CURVCHK(hipStreamSynchronize(st));
	return 0;
}
#undef CURVCHK
#undef CURVMEM
