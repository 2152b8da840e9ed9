// pga_pan_curves (include/pangene_hip.h): accumulation curves on the device (k_curves.hpp).  Context-free: it runs on a stream of
// its own on the current device.  The device buffers are kept from call to call and only ever grow (a hipMalloc per call would cost
// more than the kernels); pga_host_trim(0) gives them back.  The result waits in a host vector of the library until the next call.

namespace {
struct CurvesBuf { enum { BITS, ORD, RANK, CNT, LEN, OFF, LIST, TILES, HIST, OUT, N_BUF }; };
static_assert(CurvesBuf::N_BUF <= PAN_MAX_DEV, "the pool has room");
std::vector<int32_t> g_curves_out; // the result, under the pool's lock
}

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
	PanDev &m = g_pan[PAN_CURVES];
	std::lock_guard<std::mutex> lk(m.mu);
	g_curves_out.assign((size_t)4 * n * A, 0);
	out->count = g_curves_out.data();
	if (G == 0 || A == 0 || n == 0) return 0;
	const int32_t W = (A + 31) / 32;
	int32_t T = 2;
	while ((int64_t)T * T < 2 * (int64_t)A) ++T; // ceil(sqrt(2A))
	const int64_t list_max = (int64_t)G * std::min(T, A);
	if (list_max >= INT32_MAX || (int64_t)n * 3 * (A + 1) >= INT32_MAX || (int64_t)n * A >= INT32_MAX / 4) return PGA_ERR_RANGE;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_bits = m.get<uint32_t>(CurvesBuf::BITS, (size_t)G * W);
	int32_t *d_ord = m.get<int32_t>(CurvesBuf::ORD, (size_t)n * A), *d_rank = m.get<int32_t>(CurvesBuf::RANK, (size_t)n * A);
	int32_t *d_cnt = m.get<int32_t>(CurvesBuf::CNT, (size_t)G), *d_len = m.get<int32_t>(CurvesBuf::LEN, (size_t)G), *d_off = m.get<int32_t>(CurvesBuf::OFF, (size_t)G);
	int32_t *d_list = m.get<int32_t>(CurvesBuf::LIST, (size_t)list_max);
	I32 *d_tiles = m.get<I32>(CurvesBuf::TILES, (size_t)scan_tiles(G));
	int32_t *d_hist = m.get<int32_t>(CurvesBuf::HIST, (size_t)n * 3 * (A + 1)), *d_out = m.get<int32_t>(CurvesBuf::OUT, (size_t)4 * n * A);
	PANMEM(d_bits); PANMEM(d_ord); PANMEM(d_rank); PANMEM(d_cnt); PANMEM(d_len); PANMEM(d_off); PANMEM(d_list); PANMEM(d_tiles); PANMEM(d_hist); PANMEM(d_out);
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * (size_t)G * W, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_ord, in->order, sizeof(int32_t) * (size_t)n * A, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_hist, 0, sizeof(int32_t) * (size_t)n * 3 * (A + 1), st));
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
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(g_curves_out.data(), d_out, sizeof(int32_t) * g_curves_out.size(), hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
