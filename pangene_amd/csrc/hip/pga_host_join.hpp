// pga_pan_join (include/pangene_hip.h): the joins of pangene tree on the device (k_join.hpp).  Context-free: it runs on a stream of
// its own on the current device.  The device buffers and the page-locked results are kept from call to call and only ever grow;
// pga_host_trim(0) gives them back.  The records wait in the page-locked buffer until the next call.
//
// The live count r is known to the host at every step, so the two launches of each join are sized and queued without reading
// anything back: n - 3 (NJ) or n - 1 (UPGMA) joins back to back, one wait at the end for the records and the range flag.

constexpr int32_t JOIN_MAX_N = 65535;

namespace {
struct JoinDev {
	std::mutex mu;
	hipStream_t st = nullptr;
	enum { D, LABEL, AUX, PART, REC, N_BUF }; // REC: the records, then one word of flag
	void *p[N_BUF] = {};
	size_t cap[N_BUF] = {};
	int64_t *host = nullptr; // page-locked: the records, then the flag
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
	int64_t *get_host(size_t n)
	{
		const size_t bytes = sizeof(int64_t) * (n ? n : 1);
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
JoinDev g_join;
}

static void join_release() { std::lock_guard<std::mutex> lk(g_join.mu); g_join.release(); }

#define JOINCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::pga_pan_join] %s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); return PGA_ERR_NO_DEVICE; } } while (0)
#define JOINMEM(p) do { if ((p) == nullptr) return PGA_ERR_NOMEM; } while (0)

// workgroups of k_join_argmin at the most: JOIN_MAX_PART, or PANGENE_JOIN_PARTS (tests: several tiles per workgroup at a small n)
static int32_t join_max_part()
{
	if (const char *s = getenv("PANGENE_JOIN_PARTS")) { const long long v = atoll(s); if (v >= 1 && v <= JOIN_MAX_PART) return (int32_t)v; }
	return JOIN_MAX_PART;
}

template <bool NJ>
static int join_queue(hipStream_t st, int32_t *d_d, int32_t n, int32_t ld, int32_t *d_label, long long *d_aux, JoinPart *d_part, long long *d_rec, int32_t *d_flag)
{
	hipLaunchKernelGGL(k_join_init<NJ>, dim3((unsigned)n), dim3(BLOCK), 0, st, d_d, n, ld, d_label, d_aux, d_flag);
	JOINCHK(hipGetLastError());
	const int32_t max_part = join_max_part();
	int32_t s = 0;
	for (int32_t r = n; r > (NJ ? 3 : 1); --r, ++s) {
		const int32_t n_tile = ((r + JOIN_CW - 1) / JOIN_CW) * ((r + JOIN_RB - 1) / JOIN_RB), n_part = std::min(n_tile, max_part);
		hipLaunchKernelGGL(k_join_argmin<NJ>, dim3((unsigned)n_part), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part);
		hipLaunchKernelGGL(k_join_update<NJ>, dim3((unsigned)((r + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part, n_part,
		                   d_rec + 6 * (size_t)s, d_flag);
		if ((s & 255) == 255) JOINCHK(hipGetLastError());
	}
	if (NJ) hipLaunchKernelGGL(k_join_final, dim3(1), dim3(WAVE), 0, st, d_d, ld, d_label, d_rec + 6 * (size_t)s);
	JOINCHK(hipGetLastError());
	return 0;
}

extern "C" int pga_pan_join(const pga_join_in_t *in, pga_join_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->rec = nullptr, out->n_rec = 0;
	if (in == nullptr || in->q == nullptr || in->n < 3 || (in->method != 0 && in->method != 1)) return PGA_ERR_ARG;
	const int32_t n = in->n;
	if (n > JOIN_MAX_N) return PGA_ERR_RANGE;
	const bool nj = in->method == 0;
	const int32_t n_rec = nj ? n - 2 : n - 1, ld = (n + 3) & ~3;
	std::lock_guard<std::mutex> lk(g_join.mu);
	JoinDev &m = g_join;
	int64_t *h_rec = m.get_host(6 * (size_t)n_rec + 1);
	JOINMEM(h_rec);
	if (m.st == nullptr) JOINCHK(hipStreamCreateWithFlags(&m.st, hipStreamNonBlocking));
	hipStream_t st = m.st;
	int32_t *d_d = m.get<int32_t>(JoinDev::D, (size_t)n * (size_t)ld), *d_label = m.get<int32_t>(JoinDev::LABEL, (size_t)n);
	long long *d_aux = m.get<long long>(JoinDev::AUX, (size_t)n), *d_rec = m.get<long long>(JoinDev::REC, 6 * (size_t)n_rec + 1);
	JoinPart *d_part = m.get<JoinPart>(JoinDev::PART, JOIN_MAX_PART);
	JOINMEM(d_d); JOINMEM(d_label); JOINMEM(d_aux); JOINMEM(d_rec); JOINMEM(d_part);
	int32_t *d_flag = (int32_t *)(d_rec + 6 * (size_t)n_rec);
	if (ld == n) JOINCHK(hipMemcpyAsync(d_d, in->q, sizeof(int32_t) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, st));
	else JOINCHK(hipMemcpy2DAsync(d_d, sizeof(int32_t) * (size_t)ld, in->q, sizeof(int32_t) * (size_t)n, sizeof(int32_t) * (size_t)n, (size_t)n, hipMemcpyHostToDevice, st));
	JOINCHK(hipMemsetAsync(d_flag, 0, sizeof(long long), st));
	const int rc = nj ? join_queue<true>(st, d_d, n, ld, d_label, d_aux, d_part, d_rec, d_flag) : join_queue<false>(st, d_d, n, ld, d_label, d_aux, d_part, d_rec, d_flag);
	if (rc != 0) { (void)hipStreamSynchronize(st); return rc; }
	JOINCHK(hipMemcpyAsync(h_rec, d_rec, sizeof(int64_t) * (6 * (size_t)n_rec + 1), hipMemcpyDeviceToHost, st));
	JOINCHK(hipStreamSynchronize(st));
	if ((int32_t)h_rec[6 * (size_t)n_rec] != 0) return PGA_ERR_RANGE;
	out->rec = h_rec, out->n_rec = n_rec;
	return 0;
}
#undef JOINCHK
#undef JOINMEM
