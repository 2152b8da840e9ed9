// pga_pan_shared (include/pangene_hip.h): the shared-item matrix of pangene dist on the device (k_dist.hpp).  Context-free: it runs
// on a stream of its own on the current device.  The device buffers and the page-locked result are kept from call to call and only
// ever grow; pga_host_trim(0) gives them back.  The result waits in the page-locked buffer until the next call.

constexpr int32_t DIST_MAX_ASM = 65535;

struct DistBuf { enum { BITS, OUT, N_BUF }; };

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
	PanDev &m = g_pan[PAN_DIST];
	std::lock_guard<std::mutex> lk(m.mu);
	const size_t nn = (size_t)A * (size_t)A;
	int32_t *h_out = m.get_host<int32_t>(0, nn);
	PANMEM(h_out);
	out->shared = h_out;
	if (A == 0) return 0;
	if (W == 0) { memset(h_out, 0, sizeof(int32_t) * nn); return 0; }
	const DistShape sh = dist_shape(A, W);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_bits = m.get<uint32_t>(DistBuf::BITS, (size_t)A * (size_t)W);
	int32_t *d_out = m.get<int32_t>(DistBuf::OUT, nn);
	PANMEM(d_bits); PANMEM(d_out);
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * (size_t)A * (size_t)W, hipMemcpyHostToDevice, st));
	if (sh.n_split > 1) PANCHK(m, hipMemsetAsync(d_out, 0, sizeof(int32_t) * nn, st));
	hipLaunchKernelGGL(k_dist_shared, dim3((unsigned)sh.n_tile * (unsigned)sh.n_split), dim3(BLOCK), 0, st, d_bits, A, W, sh.n_chunk, sh.n_split, sh.cps, d_out);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_out, d_out, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
