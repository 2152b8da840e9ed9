// pga_call_bubbles (include/pangene_hip.h): the walk side of pangene.js call on the device (k_call.hpp).  Context-free: it runs on
// a stream of its own on the current device, allocates what it needs for the call and frees it before it returns; the results
// wait in host vectors of the library until the next call.

namespace {
struct CallBufs { // device allocations of one call
	std::vector<void *> p;
	~CallBufs() { for (void *x : p) (void)hipFree(x); }
	template <class T> T *get(size_t n) { void *x = nullptr; if (hipMalloc(&x, sizeof(T) * (n ? n : 1)) != hipSuccess) return nullptr; p.push_back(x); return (T *)x; }
};
struct CallHost { std::vector<int4> rec; std::vector<int32_t> rep, cnt, gbub, gseg; std::vector<uint32_t> gfirst32; std::vector<int64_t> gfirst; };
CallHost g_call;
int bits_for(uint64_t n) { int b = 1; while (b < 64 && (1ull << b) < n) ++b; return b; } // keys below n fit in b bits
}

#define CALLCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, "[E::pga_call] %s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); if (st) (void)hipStreamDestroy(st); return PGA_ERR_NO_DEVICE; } } while (0)
#define CALLMEM(p) do { if ((p) == nullptr) { if (st) (void)hipStreamDestroy(st); return PGA_ERR_NOMEM; } } while (0)

extern "C" int pga_call_bubbles(const pga_call_in_t *in, pga_call_out_t *out)
{
	memset(out, 0, sizeof(*out));
	const int64_t N = in->n_walk > 0 ? in->walk_off[in->n_walk] : 0;
	const int32_t nv = 2 * in->n_seg;
	if (in->n_walk < 0 || in->n_seg < 0 || in->n_bub < 0 || N >= INT32_MAX) return PGA_ERR_RANGE;
	// (bubble, orientation)s by end vertex, ordered by bubble * 2 + orientation
	std::vector<int32_t> eoff((size_t)nv + 2, 0), ebo, est;
	for (int32_t b = 0; b < in->n_bub; ++b) {
		if (in->bub_vs[b] < 0) continue;
		if (in->bub_vs[b] >= nv || in->bub_ve[b] < 0 || in->bub_ve[b] >= nv) return PGA_ERR_ARG;
		++eoff[(size_t)in->bub_ve[b] + 1], ++eoff[(size_t)(in->bub_vs[b] ^ 1) + 1];
	}
	for (int32_t v = 0; v < nv; ++v) eoff[(size_t)v + 1] += eoff[(size_t)v];
	ebo.resize((size_t)eoff[(size_t)nv]), est.resize((size_t)eoff[(size_t)nv]);
	{
		std::vector<int32_t> fill(eoff.begin(), eoff.end() - 1);
		for (int32_t b = 0; b < in->n_bub; ++b) {
			if (in->bub_vs[b] < 0) continue;
			int32_t k = fill[(size_t)in->bub_ve[b]]++;
			ebo[(size_t)k] = b * 2, est[(size_t)k] = in->bub_vs[b];
			k = fill[(size_t)(in->bub_vs[b] ^ 1)]++;
			ebo[(size_t)k] = b * 2 + 1, est[(size_t)k] = in->bub_ve[b] ^ 1;
		}
	}
	for (int64_t g = 0; g < N; ++g) if (in->step[g] < 0 || in->step[g] >= nv) return PGA_ERR_ARG;
	g_call = CallHost();
	if (N == 0 || ebo.empty()) return 0;
	int hb = 32;
	if (const char *e = getenv("PANGENE_CALL_HASH_BITS")) { const int x = atoi(e); if (x >= 1 && x <= 32) hb = x; }

	hipStream_t st = nullptr;
	CALLCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
	CallBufs m;
	const int64_t W = in->n_walk;
	int32_t *d_step = m.get<int32_t>((size_t)N), *d_wid = m.get<int32_t>((size_t)N), *d_cnt = m.get<int32_t>((size_t)N), *d_off = m.get<int32_t>((size_t)N);
	int64_t *d_woff = m.get<int64_t>((size_t)W + 1);
	int32_t *d_eoff = m.get<int32_t>(eoff.size()), *d_ebo = m.get<int32_t>(ebo.size()), *d_est = m.get<int32_t>(est.size());
	CALLMEM(d_step); CALLMEM(d_wid); CALLMEM(d_cnt); CALLMEM(d_off); CALLMEM(d_woff); CALLMEM(d_eoff); CALLMEM(d_ebo); CALLMEM(d_est);
	CALLCHK(hipMemcpyAsync(d_step, in->step, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, st));
	CALLCHK(hipMemcpyAsync(d_woff, in->walk_off, sizeof(int64_t) * (size_t)(W + 1), hipMemcpyHostToDevice, st));
	CALLCHK(hipMemcpyAsync(d_eoff, eoff.data(), sizeof(int32_t) * eoff.size(), hipMemcpyHostToDevice, st));
	CALLCHK(hipMemcpyAsync(d_ebo, ebo.data(), sizeof(int32_t) * ebo.size(), hipMemcpyHostToDevice, st));
	CALLCHK(hipMemcpyAsync(d_est, est.data(), sizeof(int32_t) * est.size(), hipMemcpyHostToDevice, st));

	// sort buffers, grown as later steps need more
	int64_t cap = 0;
	uint64_t *k0 = nullptr, *k1 = nullptr; uint32_t *v0 = nullptr, *v1 = nullptr, *table = nullptr; int32_t *tiles = nullptr;
	auto sort_room = [&](int64_t n) -> bool {
		if (n <= cap) return true;
		cap = n;
		k0 = m.get<uint64_t>((size_t)n), k1 = m.get<uint64_t>((size_t)n), v0 = m.get<uint32_t>((size_t)n), v1 = m.get<uint32_t>((size_t)n);
		table = m.get<uint32_t>((size_t)rs_table_len(n)), tiles = m.get<int32_t>((size_t)std::max<int64_t>(256, scan_tiles(n)) + 64);
		return k0 && k1 && v0 && v1 && table && tiles;
	};
	auto grid = [](int64_t n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); };
	auto total_of = [&](const int32_t *cnt, const int32_t *off, int64_t n, int64_t *tot) -> hipError_t { // exclusive scan's total
		int32_t a = 0, b = 0;
		hipError_t e = hipMemcpyAsync(&a, cnt + n - 1, 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipMemcpyAsync(&b, off + n - 1, 4, hipMemcpyDeviceToHost, st);
		if (e == hipSuccess) e = hipStreamSynchronize(st);
		*tot = (int64_t)a + b;
		return e;
	};
	if (!sort_room(N)) { (void)hipStreamDestroy(st); return PGA_ERR_NOMEM; }

	// 1. the per-walk index: (walk, vertex) -> positions
	const int vb = bits_for((uint64_t)nv);
	hipLaunchKernelGGL(k_call_keys, grid(N), dim3(BLOCK), 0, st, d_step, d_woff, (int32_t)W, N, vb, d_wid, k0, v0);
	uint64_t *ks; uint32_t *vs;
	device_radix_sort(k0, v0, N, vb + bits_for((uint64_t)W), RadixBufs{k1, v1, table, tiles}, &ks, &vs, st);
	const CallIdx ix{ks, vs, N, vb, d_eoff, d_ebo, d_est};
	// 2. records: count, scan, emit
	hipLaunchKernelGGL(k_call_count, grid(N), dim3(BLOCK), 0, st, ix, d_step, d_wid, d_cnt);
	device_scan(InI32{d_cnt}, OutExclI32{d_off}, N, (I32 *)tiles, OpSum{}, I32{0}, st);
	int64_t R = 0;
	CALLCHK(total_of(d_cnt, d_off, N, &R));
	if (R < 0 || R >= INT32_MAX) { (void)hipStreamDestroy(st); return PGA_ERR_RANGE; }
	if (R == 0) { CALLCHK(hipStreamSynchronize(st)); (void)hipStreamDestroy(st); return 0; }
	int4 *d_rec = m.get<int4>((size_t)R), *d_rec2 = m.get<int4>((size_t)R);
	int32_t *d_rep = m.get<int32_t>((size_t)R), *d_rcnt = m.get<int32_t>((size_t)R), *d_run = m.get<int32_t>((size_t)R), *d_nint = m.get<int32_t>((size_t)R), *d_ioff = m.get<int32_t>((size_t)R);
	CALLMEM(d_rec); CALLMEM(d_rec2); CALLMEM(d_rep); CALLMEM(d_rcnt); CALLMEM(d_run); CALLMEM(d_nint); CALLMEM(d_ioff);
	hipLaunchKernelGGL(k_call_emit, grid(N), dim3(BLOCK), 0, st, ix, d_step, d_wid, d_woff, d_off, d_rec);
	// 3. stably by bubble: (bubble, walk, en_off, st_off, orientation)
	if (!sort_room(R)) { (void)hipStreamDestroy(st); return PGA_ERR_NOMEM; }
	const int bbits = bits_for((uint64_t)in->n_bub);
	hipLaunchKernelGGL(k_call_bub_keys, grid(R), dim3(BLOCK), 0, st, d_rec, R, k0, v0);
	device_radix_sort(k0, v0, R, bbits, RadixBufs{k1, v1, table, tiles}, &ks, &vs, st);
	hipLaunchKernelGGL(k_call_gather, grid(R), dim3(BLOCK), 0, st, d_rec, vs, R, d_rec2);
	// 4. alleles
	hipLaunchKernelGGL(k_call_hash, grid(R), dim3(BLOCK), 0, st, d_rec2, R, d_step, d_woff, hb, k0, v0, d_nint);
	device_radix_sort(k0, v0, R, hb + bbits, RadixBufs{k1, v1, table, tiles}, &ks, &vs, st);
	device_scan(CallRunHead{ks}, OutInclI32{d_run}, R, (I32 *)tiles, OpMax{}, I32{0}, st);
	CALLCHK(hipMemsetAsync(d_rcnt, 0, sizeof(int32_t) * (size_t)R, st));
	hipLaunchKernelGGL(k_call_rep, grid(R), dim3(BLOCK), 0, st, d_rec2, vs, d_run, R, d_step, d_woff, d_rep, d_rcnt);
	// 5. genes
	device_scan(InI32{d_nint}, OutExclI32{d_ioff}, R, (I32 *)tiles, OpSum{}, I32{0}, st);
	int64_t I = 0;
	CALLCHK(total_of(d_nint, d_ioff, R, &I));
	if (I < 0 || I >= INT32_MAX) { (void)hipStreamDestroy(st); return PGA_ERR_RANGE; }
	int64_t H = 0;
	int32_t *d_gbub = nullptr, *d_gseg = nullptr; uint32_t *d_gfirst = nullptr;
	if (I > 0) {
		if (!sort_room(I)) { (void)hipStreamDestroy(st); return PGA_ERR_NOMEM; }
		int32_t *d_hoff = m.get<int32_t>((size_t)I);
		CALLMEM(d_hoff);
		hipLaunchKernelGGL(k_call_interior, grid(R), dim3(BLOCK), 0, st, d_rec2, R, d_ioff, d_step, d_woff, (int64_t)in->n_seg, k0, v0);
		device_radix_sort(k0, v0, I, bits_for((uint64_t)in->n_bub * (uint64_t)std::max(1, in->n_seg)), RadixBufs{k1, v1, table, tiles}, &ks, &vs, st);
		device_scan(CallKeyHead{ks}, OutExclI32{d_hoff}, I, (I32 *)tiles, OpSum{}, I32{0}, st);
		// the number of heads: exclusive offset of the last key + its own head flag
		int32_t last_off = 0; uint64_t kl = 0, kp = 0;
		CALLCHK(hipMemcpyAsync(&last_off, d_hoff + I - 1, 4, hipMemcpyDeviceToHost, st));
		CALLCHK(hipMemcpyAsync(&kl, ks + I - 1, 8, hipMemcpyDeviceToHost, st));
		if (I > 1) CALLCHK(hipMemcpyAsync(&kp, ks + I - 2, 8, hipMemcpyDeviceToHost, st));
		CALLCHK(hipStreamSynchronize(st));
		H = (int64_t)last_off + ((I == 1 || kl != kp) ? 1 : 0);
		d_gbub = m.get<int32_t>((size_t)H), d_gseg = m.get<int32_t>((size_t)H), d_gfirst = m.get<uint32_t>((size_t)H);
		CALLMEM(d_gbub); CALLMEM(d_gseg); CALLMEM(d_gfirst);
		hipLaunchKernelGGL(k_call_genes, grid(I), dim3(BLOCK), 0, st, ks, vs, I, d_hoff, (int64_t)in->n_seg, d_gbub, d_gseg, d_gfirst);
	}
	// 6. results to the host
	g_call.rec.resize((size_t)R), g_call.rep.resize((size_t)R), g_call.cnt.resize((size_t)R);
	g_call.gbub.resize((size_t)H), g_call.gseg.resize((size_t)H), g_call.gfirst32.resize((size_t)H);
	CALLCHK(hipMemcpyAsync(g_call.rec.data(), d_rec2, sizeof(int4) * (size_t)R, hipMemcpyDeviceToHost, st));
	CALLCHK(hipMemcpyAsync(g_call.rep.data(), d_rep, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, st));
	CALLCHK(hipMemcpyAsync(g_call.cnt.data(), d_rcnt, sizeof(int32_t) * (size_t)R, hipMemcpyDeviceToHost, st));
	if (H > 0) {
		CALLCHK(hipMemcpyAsync(g_call.gbub.data(), d_gbub, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToHost, st));
		CALLCHK(hipMemcpyAsync(g_call.gseg.data(), d_gseg, sizeof(int32_t) * (size_t)H, hipMemcpyDeviceToHost, st));
		CALLCHK(hipMemcpyAsync(g_call.gfirst32.data(), d_gfirst, sizeof(uint32_t) * (size_t)H, hipMemcpyDeviceToHost, st));
	}
	CALLCHK(hipStreamSynchronize(st));
	(void)hipStreamDestroy(st);
	g_call.gfirst.assign(g_call.gfirst32.begin(), g_call.gfirst32.end());
	static_assert(sizeof(int4) == sizeof(pga_call_rec_t), "record layout");
	out->n_rec = R, out->rec = (const pga_call_rec_t *)g_call.rec.data(), out->rep = g_call.rep.data(), out->cnt = g_call.cnt.data();
	out->n_gene = H, out->gene_bub = g_call.gbub.data(), out->gene_seg = g_call.gseg.data(), out->gene_first = g_call.gfirst.data();
	return 0;
}
#undef CALLCHK
#undef CALLMEM
