// pga_pan_join (include/pangene_hip.h): the joins of pangene tree on the device (k_join.hpp).  Context-free: it runs on a stream of
// its own on the current device.  The device buffers and the page-locked results are kept from call to call and only ever grow;
// pga_host_trim(0) gives them back.  The records wait in the page-locked buffer until the next call.
//
// The live count r is known to the host at every step, so the two launches of each join are sized and queued without reading
// anything back: n - 3 (NJ) or n - 1 (UPGMA) joins back to back, one wait at the end for the records and the range flag.

constexpr int32_t JOIN_MAX_N = 65535;

struct JoinBuf { enum { D, LABEL, AUX, PART, REC, N_BUF }; }; // REC: the records, then one word of flag; page-locked buffer 0: the same

// workgroups of k_join_argmin at the most: JOIN_MAX_PART, or PANGENE_JOIN_PARTS (tests: several tiles per workgroup at a small n)
static int32_t join_max_part() { return (int32_t)pan_env("PANGENE_JOIN_PARTS", JOIN_MAX_PART, JOIN_MAX_PART); }

template <bool NJ>
static int join_queue(hipStream_t st, int32_t *d_d, int32_t n, int32_t ld, int32_t *d_label, long long *d_aux, JoinPart *d_part, long long *d_rec, int32_t *d_flag)
{
	hipLaunchKernelGGL(k_join_init<NJ>, dim3((unsigned)n), dim3(BLOCK), 0, st, d_d, n, ld, d_label, d_aux, d_flag);
	PANCHK(g_pan[PAN_JOIN], hipGetLastError());
	const int32_t max_part = join_max_part();
	int32_t s = 0;
	for (int32_t r = n; r > (NJ ? 3 : 1); --r, ++s) {
		const int32_t n_tile = ((r + JOIN_CW - 1) / JOIN_CW) * ((r + JOIN_RB - 1) / JOIN_RB), n_part = std::min(n_tile, max_part);
		hipLaunchKernelGGL(k_join_argmin<NJ>, dim3((unsigned)n_part), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part);
		hipLaunchKernelGGL(k_join_update<NJ>, dim3((unsigned)((r + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part, n_part,
		                   d_rec + 6 * (size_t)s, d_flag);
		if ((s & 255) == 255) PANCHK(g_pan[PAN_JOIN], hipGetLastError());
	}
	if (NJ) hipLaunchKernelGGL(k_join_final, dim3(1), dim3(WAVE), 0, st, d_d, ld, d_label, d_rec + 6 * (size_t)s);
	PANCHK(g_pan[PAN_JOIN], hipGetLastError());
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
	PanDev &m = g_pan[PAN_JOIN];
	std::lock_guard<std::mutex> lk(m.mu);
	int64_t *h_rec = m.get_host<int64_t>(0, 6 * (size_t)n_rec + 1);
	PANMEM(h_rec);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	int32_t *d_d = m.get<int32_t>(JoinBuf::D, (size_t)n * (size_t)ld), *d_label = m.get<int32_t>(JoinBuf::LABEL, (size_t)n);
	long long *d_aux = m.get<long long>(JoinBuf::AUX, (size_t)n), *d_rec = m.get<long long>(JoinBuf::REC, 6 * (size_t)n_rec + 1);
	JoinPart *d_part = m.get<JoinPart>(JoinBuf::PART, JOIN_MAX_PART);
	PANMEM(d_d); PANMEM(d_label); PANMEM(d_aux); PANMEM(d_rec); PANMEM(d_part);
	int32_t *d_flag = (int32_t *)(d_rec + 6 * (size_t)n_rec);
	if (ld == n) PANCHK(m, hipMemcpyAsync(d_d, in->q, sizeof(int32_t) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, st));
	else PANCHK(m, hipMemcpy2DAsync(d_d, sizeof(int32_t) * (size_t)ld, in->q, sizeof(int32_t) * (size_t)n, sizeof(int32_t) * (size_t)n, (size_t)n, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_flag, 0, sizeof(long long), st));
	const int rc = nj ? join_queue<true>(st, d_d, n, ld, d_label, d_aux, d_part, d_rec, d_flag) : join_queue<false>(st, d_d, n, ld, d_label, d_aux, d_part, d_rec, d_flag);
	if (rc != 0) { (void)hipStreamSynchronize(st); return rc; }
	PANCHK(m, hipMemcpyAsync(h_rec, d_rec, sizeof(int64_t) * (6 * (size_t)n_rec + 1), hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	if ((int32_t)h_rec[6 * (size_t)n_rec] != 0) return PGA_ERR_RANGE;
	out->rec = h_rec, out->n_rec = n_rec;
	return 0;
}
