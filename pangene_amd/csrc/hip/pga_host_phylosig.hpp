// pga_pan_phylosig (include/pangene_hip.h): the permutation tail of the parsimony cost on the device (k_phylosig.hpp).  Context-free: it
// runs on a stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call in the
// PAN_PHYLOSIG pool and only ever grow; pga_host_trim(0) gives them back.
//
// The host checks the program as pga_pan_gainloss does (a malformed one would index the stack out of bounds), leaf (a row of rk per push)
// and the classes, packs the program into bit words and uploads it with leaf, the classes and the items' classes and costs.  The
// permutations then go through in batches of pga_phylosig_batch(n_cls) orders: per batch k_ps_ranks makes the orders, k_ps_cost runs
// classes x permutations up passes and adds into sum, k_ps_count adds the items' counts, one after the other on the one stream.  Nothing
// is read back between the batches and the host waits once, at the end (tests that ask for cost_rows / rank_rows wait once more, after
// the first batch).
constexpr int32_t PS_BATCH = 4096;
constexpr int64_t PS_COST_BYTES = (int64_t)256 << 20; // what the cost rows of one batch may take
constexpr int32_t PS_CLS = 2;                         // classes a lane of k_ps_cost carries (DESIGN.md section 8 "Phylogenetic signal measured")

struct PhylosigBuf {
	enum { OPS, LEAF, CLS, ITEM_CLS, ITEM_COST, RK, WORK, COST, SUM, N_LE, N_GE, N_BUF };
	enum { H_IN, H_COUNT, H_SUM }; // page-locked: the packed program; n_le and n_ge; sum
};
static_assert(PhylosigBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the phylogenetic signal buffers");

extern "C" int32_t pga_phylosig_batch(int32_t n_cls)
{
	const int64_t fit = std::min<int64_t>(PS_COST_BYTES / 4 / std::max<int64_t>(n_cls, 1), PS_BATCH) / WAVE * WAVE;
	const int64_t b = pan_env("PANGENE_PHYLOSIG_BATCH", std::max<int64_t>(fit, WAVE), 1 << 20);
	return (int32_t)((b + WAVE - 1) / WAVE * WAVE);
}

template <int32_t CLS>
static void phylosig_cost_launch(hipStream_t st, int32_t depth, int32_t nb, int32_t n_cls, const uint32_t *ops, const int32_t *leaf, const uint16_t *rk, const int32_t *cls,
                                 int32_t n_op, int32_t gain, int32_t loss, int32_t nbs, int32_t B, int32_t *cost, unsigned long long *sum)
{
	const size_t lds = sizeof(int32_t) * 2 * PS_BLOCK * CLS * (size_t)std::max(depth - 1, 1); // <= 60 KiB at depth 16 and CLS 4
	hipLaunchKernelGGL(k_ps_cost<CLS>, dim3((unsigned)((nb + PS_BLOCK - 1) / PS_BLOCK), (unsigned)((n_cls + CLS - 1) / CLS)), dim3(PS_BLOCK), lds, st, ops, leaf, rk, cls, n_cls,
	                   n_op, gain, loss, nb, nbs, B, cost, sum);
}

extern "C" int pga_pan_phylosig(const pga_phylosig_in_t *in, pga_phylosig_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->n_le = out->n_ge = nullptr, out->sum = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t L = in->n_leaf, NC = in->n_cls, NI = in->n_item, n = in->n_perm;
	if (L < 0 || NC < 0 || NI < 0 || n < 0) return PGA_ERR_ARG;
	if (L > GL_MAX_LEAF || NI > GL_MAX_GENE || n > PAN_MAX_PERM) return PGA_ERR_RANGE;
	if (in->gain < 1 || in->gain > 255 || in->loss < 1 || in->loss > 255) return PGA_ERR_RANGE;
	const int32_t n_op = L > 0 ? 2 * L - 1 : 0, OW = (n_op + 31) / 32;
	if (L > 0 && (in->op == nullptr || in->leaf == nullptr)) return PGA_ERR_ARG;
	if ((NC > 0 && in->cls == nullptr) || (NI > 0 && (in->item_cls == nullptr || in->item_cost == nullptr))) return PGA_ERR_ARG;
	// the program: n_leaf pushes, no join of fewer than two entries, one entry left; the depth it needs
	int32_t depth = 0, pushed = 0, sp = 0;
	for (int32_t k = 0; k < n_op; ++k) {
		if (in->op[k] == 0) ++pushed, depth = std::max(depth, ++sp);
		else if (in->op[k] == 1 && sp >= 2) --sp;
		else return PGA_ERR_ARG;
	}
	if (n_op > 0 && (sp != 1 || pushed != L)) return PGA_ERR_ARG;
	std::vector<uint8_t> seen((size_t)L, 0); // leaf: a permutation of 0 .. n_leaf - 1
	for (int32_t k = 0; k < L; ++k) {
		const int32_t x = in->leaf[k];
		if (x < 0 || x >= L || seen[(size_t)x]) return PGA_ERR_ARG;
		seen[(size_t)x] = 1;
	}
	for (int32_t c = 0; c < NC; ++c)
		if (in->cls[c] < 1 || in->cls[c] > L - 1 || (c > 0 && in->cls[c] <= in->cls[c - 1])) return PGA_ERR_ARG;
	for (int32_t i = 0; i < NI; ++i)
		if (in->item_cls[i] < 0 || in->item_cls[i] >= NC) return PGA_ERR_ARG;
	if (depth > GL_DEPTH) return PGA_ERR_RANGE;
	PanDev &m = g_pan[PAN_PHYLOSIG];
	std::lock_guard<std::mutex> lk(m.mu);
	int32_t *h_count = m.get_host<int32_t>(PhylosigBuf::H_COUNT, 2 * (size_t)NI);
	int64_t *h_sum = m.get_host<int64_t>(PhylosigBuf::H_SUM, (size_t)NC);
	PANMEM(h_count); PANMEM(h_sum);
	out->n_le = h_count, out->n_ge = h_count + NI, out->sum = h_sum;
	memset(h_count, 0, sizeof(int32_t) * 2 * (size_t)NI);
	memset(h_sum, 0, sizeof(int64_t) * (size_t)NC);
	if (NC == 0 || NI == 0 || n == 0) return 0; // nothing to count: no launch  (NC > 0 implies L >= 2)
	uint32_t *h_in = m.get_host<uint32_t>(PhylosigBuf::H_IN, (size_t)OW);
	PANMEM(h_in);
	memset(h_in, 0, sizeof(uint32_t) * (size_t)OW);
	for (int32_t k = 0; k < n_op; ++k) h_in[k >> 5] |= (uint32_t)in->op[k] << (k & 31);
	PermBatches b(n, pga_phylosig_batch(NC), L <= PS_RANK_LDS_N);
	const int32_t B = b.B, BS = (B + WAVE - 1) / WAVE * WAVE; // rk has room for the widest batch; a batch of nb uses nbs = nb rounded up to 64 of it
	int32_t n_cls_lane = (int32_t)pan_env("PANGENE_PHYLOSIG_CLS", PS_CLS, 4); // (measurements: 1, 2 or 4 classes a lane)
	if (n_cls_lane == 3) n_cls_lane = PS_CLS;
	const bool timing = getenv("PANGENE_PHYLOSIG_TIMING") != nullptr;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_ops = m.get<uint32_t>(PhylosigBuf::OPS, (size_t)OW);
	int32_t *d_leaf = m.get<int32_t>(PhylosigBuf::LEAF, (size_t)L), *d_cls = m.get<int32_t>(PhylosigBuf::CLS, (size_t)NC);
	int32_t *d_icls = m.get<int32_t>(PhylosigBuf::ITEM_CLS, (size_t)NI), *d_icost = m.get<int32_t>(PhylosigBuf::ITEM_COST, (size_t)NI);
	uint16_t *d_rk = m.get<uint16_t>(PhylosigBuf::RK, (size_t)L * (size_t)BS), *d_work = m.get<uint16_t>(PhylosigBuf::WORK, b.work((size_t)L));
	int32_t *d_cost = m.get<int32_t>(PhylosigBuf::COST, (size_t)NC * (size_t)B);
	unsigned long long *d_sum = m.get<unsigned long long>(PhylosigBuf::SUM, (size_t)NC);
	int32_t *d_le = m.get<int32_t>(PhylosigBuf::N_LE, (size_t)NI), *d_ge = m.get<int32_t>(PhylosigBuf::N_GE, (size_t)NI);
	PANMEM(d_ops); PANMEM(d_leaf); PANMEM(d_cls); PANMEM(d_icls); PANMEM(d_icost); PANMEM(d_rk); PANMEM(d_work); PANMEM(d_cost); PANMEM(d_sum); PANMEM(d_le); PANMEM(d_ge);
	PANCHK(m, hipMemcpyAsync(d_ops, h_in, sizeof(uint32_t) * (size_t)OW, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_leaf, in->leaf, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_cls, in->cls, sizeof(int32_t) * (size_t)NC, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_icls, in->item_cls, sizeof(int32_t) * (size_t)NI, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_icost, in->item_cost, sizeof(int32_t) * (size_t)NI, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_sum, 0, sizeof(unsigned long long) * (size_t)NC, st));
	PANCHK(m, hipMemsetAsync(d_le, 0, sizeof(int32_t) * (size_t)NI, st));
	PANCHK(m, hipMemsetAsync(d_ge, 0, sizeof(int32_t) * (size_t)NI, st));
	std::vector<hipEvent_t> ev; // PANGENE_PHYLOSIG_TIMING: four per batch, around the three kernels
	auto mark = [&]() {
		if (!timing) return;
		hipEvent_t e = nullptr;
		if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, st); ev.push_back(e); }
	};
	for (; b.more(); b.next()) {
		const int32_t nb = b.nb(), nbs = (nb + WAVE - 1) / WAVE * WAVE;
		mark();
		perm_launch(b.lds, k_ps_ranks<true>, k_ps_ranks<false>, nb, st, L, in->seed, b.p0(), nbs, d_work, d_rk);
		mark();
		if (n_cls_lane == 1) phylosig_cost_launch<1>(st, depth, nb, NC, d_ops, d_leaf, d_rk, d_cls, n_op, in->gain, in->loss, nbs, B, d_cost, d_sum);
		else if (n_cls_lane == 2) phylosig_cost_launch<2>(st, depth, nb, NC, d_ops, d_leaf, d_rk, d_cls, n_op, in->gain, in->loss, nbs, B, d_cost, d_sum);
		else phylosig_cost_launch<4>(st, depth, nb, NC, d_ops, d_leaf, d_rk, d_cls, n_op, in->gain, in->loss, nbs, B, d_cost, d_sum);
		mark();
		hipLaunchKernelGGL(k_ps_count, dim3((unsigned)((NI + PS_COUNT_BLOCK / WAVE - 1) / (PS_COUNT_BLOCK / WAVE))), dim3(PS_COUNT_BLOCK), 0, st, d_cost, d_icls, d_icost, NI, nb, B,
		                   d_le, d_ge);
		mark();
		PANCHK(m, hipGetLastError());
		if (b.first() && (in->cost_rows != nullptr || in->rank_rows != nullptr)) { // tests only: the first batch's costs and orders
			if (in->cost_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->cost_rows, d_cost, sizeof(int32_t) * (size_t)NC * (size_t)nb, hipMemcpyDeviceToHost, st)); // (the first batch is the widest: nb == B)
			if (in->rank_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->rank_rows, d_rk, sizeof(uint16_t) * (size_t)L * (size_t)nbs, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
	}
	PANCHK(m, hipMemcpyAsync(h_count, d_le, sizeof(int32_t) * (size_t)NI, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_count + NI, d_ge, sizeof(int32_t) * (size_t)NI, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_sum, d_sum, sizeof(int64_t) * (size_t)NC, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	if (timing) {
		float t[3] = {0, 0, 0};
		for (size_t k = 0; k + 3 < ev.size(); k += 4)
			for (int j = 0; j < 3; ++j) { float ms = 0; if (hipEventElapsedTime(&ms, ev[k + (size_t)j], ev[k + (size_t)j + 1]) == hipSuccess) t[j] += ms; }
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
		fprintf(stderr, "[phylosig-kernels] leaves=%d classes=%d items=%d perms=%d batch=%d cls_per_lane=%d depth=%d ranks_ms=%.3f cost_ms=%.3f count_ms=%.3f\n", L, NC, NI, n, B,
		        n_cls_lane, depth, t[0], t[1], t[2]);
	}
	return 0;
}
