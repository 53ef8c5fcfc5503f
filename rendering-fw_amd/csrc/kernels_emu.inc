// kernels_emu.inc — the HOST EMULATION drivers of the work items in kernels.hip: plain loops over the same item functions (and, for
// the packet form of the primary wave, the same steps over arrays of 64 lanes), compiled by g++ with -DRFWHIP_HOST_EMULATION into
// tests/_emu/ only.  Test infrastructure for the CPU tier: build.py never defines RFWHIP_HOST_EMULATION, the product never
// includes this file's contents.  Included by kernels.hip inside namespace rtk.
// ================================================================================================================

struct Rng4
{
	uint32_t v[4];
};

void set_device_cus(int) {}
uint32_t max_lds_nodes() { return MAX_LDS_NODES; }
void launch_init_counters(WaveCounters *c, uint32_t primary_count, stream_t s)
{
	EMU_DEFER(s, launch_init_counters(c, primary_count, s));
	init_counters_item(c, primary_count, 0u, 1u);
}
void launch_set_ext_count(WaveCounters *c, uint32_t depth, uint32_t count, stream_t s)
{
	EMU_DEFER(s, launch_set_ext_count(c, depth, count, s));
	c->ext[depth] = c->ext_n[depth] = count;
}

void launch_rng_states(uint32_t *states, const uint32_t base_state[4], const uint32_t *jump_table,
					   uint32_t packets_per_sample, uint32_t spp, stream_t s)
{
	const Rng4 base{{base_state[0], base_state[1], base_state[2], base_state[3]}}; // (a host array: taken at enqueue)
	EMU_DEFER(s, launch_rng_states(states, base.v, jump_table, packets_per_sample, spp, s));
	const uint32_t total = packets_per_sample * spp;
	for (uint32_t r = 0; r < (total + RNG_RUN - 1) / RNG_RUN; r++)
		rng_states_item(states, base_state, jump_table, total, r);
}

// ---- the packet form of the pt primary wave (device: trace_packet / k_primary_packet), one wave = 64 array entries ---------------
// The same steps in the same order with the same arithmetic — ballots are loops, v_readlane / v_writelane are array accesses —
// so that the CPU tier checks the algorithm (stack discipline, partial child order, mixed direction signs, instances) against
// the per-lane traversal and the oracle.
namespace packet_emu
{
constexpr int WAVE = 64;
struct Space
{
	f3 o[WAVE], d[WAVE], id[WAVE], noid[WAVE];
	uint32_t off_n[3], off_f[3];
	bool mixed;
	void enter(const f3 *o_, const f3 *d_, const Hit *hit, unsigned long long act)
	{
		unsigned long long mx = 0, my = 0, mz = 0;
		for (int l = 0; l < WAVE; l++)
		{
			o[l] = o_[l], d[l] = d_[l];
			id[l] = mk3(slab_rcp(d[l].x), slab_rcp(d[l].y), slab_rcp(d[l].z));
			id[l] = id[l] * norm_k(hit[l].t);
			noid[l] = mk3(-(o[l].x * id[l].x), -(o[l].y * id[l].y), -(o[l].z * id[l].z));
			mx |= (unsigned long long)(id[l].x < 0.0f) << l, my |= (unsigned long long)(id[l].y < 0.0f) << l, mz |= (unsigned long long)(id[l].z < 0.0f) << l;
		}
		mx &= act, my &= act, mz &= act;
		mixed = (mx != 0ull && mx != act) || (my != 0ull && my != act) || (mz != 0ull && mz != act);
		off_n[0] = mx ? 48u : 0u, off_f[0] = mx ? 0u : 48u;
		off_n[1] = my ? 64u : 16u, off_f[1] = my ? 16u : 64u;
		off_n[2] = mz ? 80u : 32u, off_f[2] = mz ? 32u : 80u;
	}
};
struct Stack
{
	uint32_t s0[WAVE];
	uint32_t sp = 1u;
	Stack()
	{
		for (int l = 0; l < WAVE; l++)
			s0[l] = 0u;
		s0[0] = ENTRY_DONE;
	}
	void push(uint32_t e) { s0[sp++ & 63u] = e; }
	uint32_t pop() { return s0[--sp & 63u]; }
	void push3(uint32_t ea, uint32_t na, uint32_t eb, uint32_t nb, uint32_t ec, uint32_t nc)
	{
		s0[sp & 63u] = ea, s0[(sp + na) & 63u] = eb, s0[(sp + na + nb) & 63u] = ec;
		sp += na + nb + nc;
	}
};
#if defined(RT_DEV_PACKET_COST)
// development (tools/dev/packet_cost.py): what the WAVE walks — node steps and leaf triangle tests per launch of the primary wave,
// whatever the per-ray counters say; RT_DEV_ORDER_PLANB=1 in the environment: the ordered walk with one comparator (DESIGN_LOG.md)
static unsigned long long g_cost_nodes = 0, g_cost_tris = 0;
#endif
// ORDERED: the node table holds every node's children near to far as seen from the camera (primary_order.h) — they are taken as
// they come (device: trace_packet<COUNT, false, true>, k_primary_packet; ORDERED = false: k_primary_packet_sorting)
// entry (ORDERED; null: the root): the group's record of the entry snapshot (primary_entry.h), where the walk starts
template <bool COUNT, bool ORDERED = false>
void trace(const SceneView &sc, const bool *active, const f3 *O, const f3 *D, float t_min, Hit *hit, TStat &st, const uint32_t *entry = nullptr)
{
	unsigned long long act = 0;
	for (int l = 0; l < WAVE; l++)
	{
		act |= (unsigned long long)active[l] << l;
		hit[l].t = active[l] ? hit[l].t : -3.0e38f;
	}
	if (act == 0ull)
		return;
	int ref_lane = 0;
	while (!((act >> ref_lane) & 1ull))
		ref_lane++;
	uint32_t nact = 0;
	for (int l = 0; l < WAVE; l++)
		nact += active[l] ? 1u : 0u;
	static thread_local Space sp;
	sp.enter(O, D, hit, act);
	Stack stk;
	int cur_inst = -1;
	uint32_t cur = sc.instance_count ? sc.tlas_root_entry : ENTRY_DONE;
	if (ORDERED && entry) // (device: lane j + 1 takes word j, sp from a ballot of the used words)
	{
		for (uint32_t j = 0; j < PRIMARY_ENTRY_K; j++)
		{
			stk.s0[j + 1u] = entry[j];
			stk.sp += entry[j] != ENTRY_DONE ? 1u : 0u;
		}
		cur = stk.pop();
	}
	if (COUNT && cur != ENTRY_DONE)
	{
		if (!(cur & ENTRY_LEAF))
			st.inner += nact;
		else if (!(cur & ENTRY_TLAS))
			st.tris += nact * (((cur >> 27) & 7u) + 1u);
	}
	const char *const nodes = (const char *)sc.nodes4f;
	for (;;)
	{
		while (!(cur & ENTRY_LEAF))
		{
			const Node4f &nd = *(const Node4f *)(nodes + ((size_t)(cur & ENTRY_INDEX_MASK) << 7));
			float tk_ref[4];
			unsigned long long m[4];
			for (int k = 0; k < 4; k++)
			{
				m[k] = 0ull;
				for (int l = 0; l < WAVE; l++)
				{
					float tmin, tmax;
					if (!sp.mixed)
					{
						const float *nx = (const float *)((const char *)&nd + sp.off_n[0]), *ny = (const float *)((const char *)&nd + sp.off_n[1]);
						const float *nz = (const float *)((const char *)&nd + sp.off_n[2]), *fx = (const float *)((const char *)&nd + sp.off_f[0]);
						const float *fy = (const float *)((const char *)&nd + sp.off_f[1]), *fz = (const float *)((const char *)&nd + sp.off_f[2]);
						tmin = fmaxf(fmaxf(fmaf(nx[k], sp.id[l].x, sp.noid[l].x), fmaf(ny[k], sp.id[l].y, sp.noid[l].y)), fmaf(nz[k], sp.id[l].z, sp.noid[l].z));
						tmax = fminf(fminf(fmaf(fx[k], sp.id[l].x, sp.noid[l].x), fmaf(fy[k], sp.id[l].y, sp.noid[l].y)), fmaf(fz[k], sp.id[l].z, sp.noid[l].z));
					}
					else
					{
						const float ax = fmaf(nd.lo[0][k], sp.id[l].x, sp.noid[l].x), bx = fmaf(nd.hi[0][k], sp.id[l].x, sp.noid[l].x);
						const float ay = fmaf(nd.lo[1][k], sp.id[l].y, sp.noid[l].y), by = fmaf(nd.hi[1][k], sp.id[l].y, sp.noid[l].y);
						const float az = fmaf(nd.lo[2][k], sp.id[l].z, sp.noid[l].z), bz = fmaf(nd.hi[2][k], sp.id[l].z, sp.noid[l].z);
						tmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
						tmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
					}
					// (normalised distances: the interval a box must meet is [0, 1] — device: v_max3 / v_min3 with the clamp modifier)
					const float tk = fminf(fmaxf(tmin, 0.0f), 1.0f);
					tmax = fminf(fmaxf(tmax, 0.0f), 1.0f);
					if (l == ref_lane)
						tk_ref[k] = tk;
					if (tk < tmax && ((act >> l) & 1ull))
						m[k] |= 1ull << l;
				}
				if (sp.mixed && nd.entry[k] == ENTRY_EMPTY)
					m[k] = 0ull;
			}
			if (COUNT)
				for (int k = 0; k < 4; k++) // per ray: the children IT enters (device: trace_packet)
				{
					const uint32_t e = nd.entry[k];
					uint32_t n = 0;
					for (int l = 0; l < WAVE; l++)
						n += (uint32_t)((m[k] >> l) & 1ull);
					if (!(e & ENTRY_LEAF))
						st.inner += n;
					else if (!(e & ENTRY_TLAS))
						st.tris += n * (((e >> 27) & 7u) + 1u);
				}
#if defined(RT_DEV_PACKET_COST)
			g_cost_nodes++;
			static const bool planb = getenv("RT_DEV_ORDER_PLANB") && atoi(getenv("RT_DEV_ORDER_PLANB")) != 0;
#else
			constexpr bool planb = false;
#endif
			// (ORDERED: no keys — an entered child's is 0, the children stay as the table has them)
			uint32_t kk[4], ee[4];
			for (int k = 0; k < 4; k++)
				kk[k] = m[k] ? (ORDERED && !(planb && k < 2) ? 0u : fbits(tk_ref[k])) : 0xFFFFFFFFu, ee[k] = nd.entry[k];
			auto pswap = [&](int a, int b) {
				if (kk[b] < kk[a])
				{
					const uint32_t tk_ = kk[a], te_ = ee[a];
					kk[a] = kk[b], ee[a] = ee[b], kk[b] = tk_, ee[b] = te_;
				}
			};
			if (!ORDERED)
				pswap(0, 1), pswap(2, 3), pswap(0, 2);
			else if (planb)
				pswap(0, 1);
			stk.push3(ee[3], kk[3] != 0xFFFFFFFFu, ee[2], kk[2] != 0xFFFFFFFFu, ee[1], kk[1] != 0xFFFFFFFFu);
			cur = kk[0] != 0xFFFFFFFFu ? ee[0] : stk.pop();
		}
		if (cur == ENTRY_DONE)
			break;
		if (cur == ENTRY_SENTINEL)
		{
			sp.enter(O, D, hit, act);
			cur_inst = -1;
			cur = stk.pop();
			continue;
		}
		if (cur & ENTRY_TLAS)
		{
			const uint32_t ii = sc.tlas_prims[cur & ENTRY_FIRST_MASK];
			const Instance &in = sc.instances[ii];
			stk.push(ENTRY_SENTINEL);
			static thread_local f3 o2[WAVE], d2[WAVE];
			for (int l = 0; l < WAVE; l++)
			{
				o2[l] = mk3(row_point_r(in.inv, O[l]), row_point_r(in.inv + 4, O[l]), row_point_r(in.inv + 8, O[l]));
				d2[l] = mk3(row_dir_r(in.inv, D[l]), row_dir_r(in.inv + 4, D[l]), row_dir_r(in.inv + 8, D[l]));
			}
			sp.enter(o2, d2, hit, act);
			cur_inst = (int)ii;
			cur = in.root_entry;
			continue;
		}
		{
			const uint32_t first = cur & ENTRY_FIRST_MASK, count = ((cur >> 27) & 7u) + 1u;
#if defined(RT_DEV_PACKET_COST)
			g_cost_tris += count;
#endif
			float t_before[WAVE];
			for (int l = 0; l < WAVE; l++)
				t_before[l] = hit[l].t;
			for (uint32_t i = 0; i < count; i++)
			{
				const f4 *tv = sc.tri_verts + 3u * (first + i);
				const f4 v0 = tv[0], v1 = tv[1], v2 = tv[2];
				const int tri_inst = cur_inst >= 0 ? cur_inst : (int)fbits(v1.w);
				for (int l = 0; l < WAVE; l++)
					if (tri_test<true>(sp.o[l], sp.d[l], t_min, hit[l].t, xyz(v0), xyz(v1), xyz(v2), hit[l].u, hit[l].v, v2.w, fbits(v0.w), (uint32_t)hit[l].prim,
									   (uint32_t)tri_inst, (uint32_t)hit[l].inst))
					{
						hit[l].prim = (int)fbits(v0.w);
						hit[l].inst = tri_inst;
					}
			}
			for (int l = 0; l < WAVE; l++)
				if (hit[l].t != t_before[l])
				{
					const float r = norm_k(hit[l].t) * fast_rcp(norm_k(t_before[l])) * 0.99999952f;
					sp.id[l] = sp.id[l] * r, sp.noid[l] = sp.noid[l] * r;
				}
			cur = stk.pop();
		}
	}
}
// mask (adaptive.h): one byte per slot tile, null = every tile is traced
template <bool COUNT, bool ORDERED = false> void primary(const Params &p, uint32_t count, const unsigned char *mask = nullptr)
{
	TStat st;
	st.inner = 0, st.tris = 0, st.lds = 0;
	unsigned long long nrays = 0;
	for (uint32_t base = 0; base < count; base += WAVE)
	{
		if (mask && !mask[ad_slot_tile(p.fr, base)]) // (a retired tile's group: void records, nothing traced)
		{
			for (uint32_t idx = base; idx < base + WAVE && idx < count; idx++)
				p.wv.hit0[idx] = ad_void_hit();
			if (p.wv.hit0_done)
				p.wv.hit0_done[base >> 6] = 1;
			continue;
		}
		bool active[WAVE];
		f3 O[WAVE], D[WAVE];
		Hit h[WAVE];
		for (int l = 0; l < WAVE; l++)
		{
			const uint32_t idx = base + (uint32_t)l;
			active[l] = idx < count;
			O[l] = mk3(0, 0, 0), D[l] = mk3(0, 0, 1);
			if (active[l])
			{
				const PixelRef pr = slot_to_pixel(p.fr, idx);
				active[l] = pr.valid;
				if (active[l])
					pt_primary_ray(p.cam, p.fr, pr.x, pr.y, p.fr.sample_base + pr.sample, O[l], D[l]);
			}
			h[l].t = 1e34f, h[l].u = 0.0f, h[l].v = 0.0f, h[l].prim = -1, h[l].inst = -1;
		}
		const uint32_t *entry = nullptr; // (device: primary_packet_body.h)
		if (ORDERED && !COUNT && p.wv.primary_entry)
			entry = p.wv.primary_entry + (size_t)((base - fast_div(base, p.fr.div_group) * (p.fr.slots << p.fr.sgroup_log2)) >> 6) * PRIMARY_ENTRY_K;
		trace<COUNT, ORDERED>(p.sc, active, O, D, 1e-5f, h, st, entry);
		for (int l = 0; l < WAVE; l++)
			if (active[l])
			{
				primary_finish_item(p, base + (uint32_t)l, D[l], h[l]);
				nrays++;
			}
	}
#if defined(RT_DEV_PACKET_COST)
	fprintf(stderr, "packet_cost ordered=%d node_steps=%llu leaf_tris=%llu\n", (int)ORDERED, g_cost_nodes, g_cost_tris);
	g_cost_nodes = g_cost_tris = 0;
#endif
	if (COUNT)
	{
		WaveCounters *const wc = p.wv.counters;
		wc->inner_extend += st.inner, wc->tris_extend += st.tris, wc->rays_extend += nrays;
	}
}
} // namespace packet_emu

bool primary_packet_form(const Params &, uint32_t) { return false; } // (the emulation keeps no group flags: every record is read)
bool primary_packet_walk(const Params &p, uint32_t max_items) { return RT_PRIMARY_PACKET_RULE(p, max_items); }

void launch_extend(const Params &p, int gen, bool count, uint32_t max_items, stream_t s, const Node4f *ordered)
{
	EMU_DEFER(s, launch_extend(p, gen, count, max_items, s, ordered));
	if (gen == GEN_PT && RT_PRIMARY_PACKET_RULE(p, max_items)) // (the device's rule)
	{
		if (ordered)
		{
			Params po = p;
			po.sc.nodes4f = ordered;
			count ? packet_emu::primary<true, true>(po, max_items) : packet_emu::primary<false, true>(po, max_items);
		}
		else
			count ? packet_emu::primary<true>(p, max_items) : packet_emu::primary<false>(p, max_items);
		return;
	}
	Ctx ctx(p);
	const uint32_t n = (gen == GEN_BUFFER || gen == GEN_RANGED) ? p.wv.counters->ext_n[p.depth] : max_items;
	for (uint32_t i = 0; i < n; i++)
	{
		if (gen == GEN_BUFFER)
			count ? extend_item<GEN_BUFFER, true>(p, i, true, ctx) : extend_item<GEN_BUFFER, false>(p, i, true, ctx);
		else if (gen == GEN_RANGED)
			count ? extend_item<GEN_RANGED, true>(p, i, true, ctx) : extend_item<GEN_RANGED, false>(p, i, true, ctx);
		else if (gen == GEN_PT)
			count ? extend_item<GEN_PT, true>(p, i, true, ctx) : extend_item<GEN_PT, false>(p, i, true, ctx);
		else
			count ? extend_item<GEN_PARITY, true>(p, i, true, ctx) : extend_item<GEN_PARITY, false>(p, i, true, ctx);
	}
}
void launch_extend_masked(const Params &p, const unsigned char *mask, bool count, uint32_t max_items, stream_t s, const Node4f *ordered)
{
	EMU_DEFER(s, launch_extend_masked(p, mask, count, max_items, s, ordered));
	if (RT_PRIMARY_PACKET_RULE(p, max_items))
	{
		if (ordered)
		{
			Params po = p;
			po.sc.nodes4f = ordered;
			count ? packet_emu::primary<true, true>(po, max_items, mask) : packet_emu::primary<false, true>(po, max_items, mask);
		}
		else
			count ? packet_emu::primary<true>(p, max_items, mask) : packet_emu::primary<false>(p, max_items, mask);
		return;
	}
	Ctx ctx(p);
	for (uint32_t i = 0; i < max_items; i++)
		count ? extend_masked_item<true>(p, mask, i, true, ctx) : extend_masked_item<false>(p, mask, i, true, ctx);
}
void launch_shade_parity(const Params &p, bool count, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_shade_parity(p, count, max_items, s));
	Ctx ctx(p);
	for (uint32_t i = 0; i < max_items; i++)
		count ? shade_parity_item<true>(p, i, true, ctx) : shade_parity_item<false>(p, i, true, ctx);
}
uint32_t queue_pad(uint32_t) { return 0u; }
void launch_shade_pt(const Params &p, const SkyView &sky, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_shade_pt(p, sky, max_items, s));
	Ctx ctx;
	const uint32_t n = p.wv.counters->ext_n[p.depth];
	const f4 *const hits = p.depth == 0 ? p.wv.hit0 : p.wv.hit;
	const int *const insts = p.depth == 0 ? p.wv.hit0_inst : p.wv.hit_inst;
	for (uint32_t i = 0; i < n; i++)
	{
		// what the device kernel's scan passes over: the padding slots of partial tiles / strips in the primary wave (their records
		// were never written), and a primary miss the packet form finished itself (primary_finish_item)
		if (p.depth == 0 && !slot_to_pixel(p.fr, i).valid)
			continue;
		const f4 h4 = hits[i];
		if ((int)fbits(h4.w) < -1)
			continue;
#if defined(RT_DIAG_SHADE_CLOCK)
		ClkProbe clk0;
		clk0.last = 0, clk0.acc = nullptr;
		if (sky.pick > 0.0f)
			p.textured ? shade_pt_item<true, true, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx, &clk0) : shade_pt_item<false, true, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx, &clk0);
		else
			p.textured ? shade_pt_item<true, false, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx, &clk0) : shade_pt_item<false, false, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx, &clk0);
#else
		// (sky sampling: what k_shade_pt_sky runs)
		if (sky.pick > 0.0f)
			p.textured ? shade_pt_item<true, true, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx) : shade_pt_item<false, true, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx);
		else
			p.textured ? shade_pt_item<true, false, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx) : shade_pt_item<false, false, false, false>(p, sky, LightTreeView{}, i, true, h4, insts[i], ctx);
#endif
	}
	p.wv.counters->ext[p.depth + 1] += ctx.q_ext.rays, p.wv.counters->shadow[p.depth] += ctx.q_shadow.rays;
}
void launch_shade_pt_lt(const Params &p, const SkyView &sky, const LightTreeView &lt, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_shade_pt_lt(p, sky, lt, max_items, s));
	Ctx ctx;
	const uint32_t n = p.wv.counters->ext_n[p.depth];
	const f4 *const hits = p.depth == 0 ? p.wv.hit0 : p.wv.hit;
	const int *const insts = p.depth == 0 ? p.wv.hit0_inst : p.wv.hit_inst;
#if defined(RT_DIAG_SHADE_CLOCK)
	ClkProbe clk0;
	clk0.last = 0, clk0.acc = nullptr;
#define RT_EMU_CLK , &clk0
#else
#define RT_EMU_CLK
#endif
	for (uint32_t i = 0; i < n; i++)
	{
		// (the entries launch_shade_pt passes over)
		if (p.depth == 0 && !slot_to_pixel(p.fr, i).valid)
			continue;
		const f4 h4 = hits[i];
		if ((int)fbits(h4.w) < -1)
			continue;
		// (what k_shade_pt_lt<TEX, SKY> runs)
		if (sky.pick > 0.0f)
			p.textured ? shade_pt_item<true, true, true, false>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK) : shade_pt_item<false, true, true, false>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK);
		else
			p.textured ? shade_pt_item<true, false, true, false>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK) : shade_pt_item<false, false, true, false>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK);
	}
#undef RT_EMU_CLK
	p.wv.counters->ext[p.depth + 1] += ctx.q_ext.rays, p.wv.counters->shadow[p.depth] += ctx.q_shadow.rays;
}
void launch_shade_pt_maps(const Params &p, const SkyView &sky, const LightTreeView &lt, bool with_lt, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_shade_pt_maps(p, sky, lt, with_lt, max_items, s));
	Ctx ctx;
	const uint32_t n = p.wv.counters->ext_n[p.depth];
	const f4 *const hits = p.depth == 0 ? p.wv.hit0 : p.wv.hit;
	const int *const insts = p.depth == 0 ? p.wv.hit0_inst : p.wv.hit_inst;
#if defined(RT_DIAG_SHADE_CLOCK)
	ClkProbe clk0;
	clk0.last = 0, clk0.acc = nullptr;
#define RT_EMU_CLK , &clk0
#else
#define RT_EMU_CLK
#endif
	for (uint32_t i = 0; i < n; i++)
	{
		// (the entries launch_shade_pt passes over)
		if (p.depth == 0 && !slot_to_pixel(p.fr, i).valid)
			continue;
		const f4 h4 = hits[i];
		if ((int)fbits(h4.w) < -1)
			continue;
		// (what k_shade_pt_maps<SKY, LT> runs)
		if (with_lt)
			sky.pick > 0.0f ? shade_pt_item<true, true, true, true>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK) : shade_pt_item<true, false, true, true>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK);
		else
			sky.pick > 0.0f ? shade_pt_item<true, true, false, true>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK) : shade_pt_item<true, false, false, true>(p, sky, lt, i, true, h4, insts[i], ctx RT_EMU_CLK);
	}
#undef RT_EMU_CLK
	p.wv.counters->ext[p.depth + 1] += ctx.q_ext.rays, p.wv.counters->shadow[p.depth] += ctx.q_shadow.rays;
}
void launch_connect(const Params &p, bool count, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_connect(p, count, max_items, s));
	Ctx ctx(p);
	const uint32_t n = connection_count(p.wv.counters, p.depth);
	if (n == 0u && p.depth == 0 && p.wv.rad_nee)
		for (uint32_t i = 0; i < p.wv.counters->shadow_n[0]; i++)
			connect_skip_item(p, i);
	for (uint32_t i = 0; i < n; i++)
		count ? connect_item<true>(p, i, true, ctx) : connect_item<false>(p, i, true, ctx);
}
void launch_shadow_packets(const Params &p, bool count, uint32_t max_items, stream_t s)
{
#if defined(RFWHIP_EMU_STREAMS) && RFWHIP_EMU_STREAMS
	if (emu_streams::deferring())
		emu_streams::state().shadow_packet_launches++; // (rfwhip_emu_schedule_stats: the packet form really was chosen)
#endif
	launch_connect(p, count, max_items, s); // (same answers per ray)
}
void launch_trace_fused(const Params &pe, const Params &pa, bool count, uint32_t max_items, stream_t s)
{
	EMU_DEFER(s, launch_trace_fused(pe, pa, count, max_items, s)); // (one launch: its two waves run together)
	launch_extend(pe, GEN_BUFFER, count, max_items, s);
	launch_connect(pa, count, max_items, s);
}
void launch_resolve(const Params &p, stream_t s)
{
	EMU_DEFER(s, launch_resolve(p, s));
	for (uint32_t i = 0; i < p.fr.W * p.fr.local_rows; i++)
		resolve_item(p, i);
}
void launch_resolve_noise(const Params &p, float *moments, uint32_t n_a, stream_t s)
{
	EMU_DEFER(s, launch_resolve_noise(p, moments, n_a, s));
	for (uint32_t i = 0; i < p.fr.W * p.fr.local_rows; i++)
		resolve_noise_item(p, moments, n_a, i);
}
uint32_t noise_tiles_x(uint32_t W) { return (W + NZ_TILE_X - 1u) / NZ_TILE_X; }
void launch_noise_merge(const float *samples_rgb, float *moments, uint32_t pixels, uint32_t n_a, uint32_t S, stream_t s)
{
	EMU_DEFER(s, launch_noise_merge(samples_rgb, moments, pixels, n_a, S, s));
	for (uint32_t i = 0; i < pixels; i++)
		nz_merge_item(samples_rgb, moments, n_a, S, i);
}
// a tile's pixels in row-major order, the tiles in index order; pixel(x, yl, e) = the kernel's pixel item
template <class Pixel> static void noise_tiles_loop(const NoiseView &v, bool final, const Pixel &pixel)
{
	const uint32_t tx = noise_tiles_x(v.W), ty = v.local_rows / NZ_TILE_Y;
	for (uint32_t k = 0; k < tx * ty; k++)
	{
		NoiseTile t = {0.0f, 0.0f, 0u, 0u};
		for (uint32_t j = 0; j < NZ_TILE_X * NZ_TILE_Y; j++)
		{
			float e;
			if (pixel((k % tx) * NZ_TILE_X + j % NZ_TILE_X, (k / tx) * NZ_TILE_Y + j / NZ_TILE_X, e))
				t.sum_e += e, t.max_e = fmaxf(t.max_e, e), t.pixels++, t.converged += e <= v.threshold;
		}
		t.sum_e = fminf(t.sum_e, FLT_MAX);
		v.tiles[k] = t;
	}
	if (final)
		nz_fold(v.tiles, tx * ty, 0u, 1u, *v.total);
}
void launch_noise_metric(const NoiseView &v, stream_t s)
{
	EMU_DEFER(s, launch_noise_metric(v, s));
	noise_tiles_loop(v, true, [&](uint32_t x, uint32_t yl, float &e) { return nz_pixel_item(v, x, yl, e); });
}
void launch_resolve_adaptive(const Params &p, float *moments, const AdaptiveView &a, stream_t s)
{
	EMU_DEFER(s, launch_resolve_adaptive(p, moments, a, s));
	for (uint32_t i = 0; i < p.fr.W * p.fr.local_rows; i++)
		resolve_adaptive_item(p, moments, a, i);
}
void launch_present_adaptive(const Params &p, f4 *out, const AdaptiveView &a, int full, stream_t s)
{
	EMU_DEFER(s, launch_present_adaptive(p, out, a, full, s));
	for (uint32_t i = 0; i < p.fr.W * p.fr.local_rows; i++)
		present_adaptive_item(p, out, a, full, i);
}
void launch_noise_metric_adaptive(const NoiseView &v, const uint32_t *n_tile, bool final, stream_t s)
{
	EMU_DEFER(s, launch_noise_metric_adaptive(v, n_tile, final, s));
	noise_tiles_loop(v, final, [&](uint32_t x, uint32_t yl, float &e) { return ad_noise_pixel_item(v, n_tile, x, yl, e); });
}
void launch_adaptive_connections(WaveCounters *c, uint32_t depth, stream_t s)
{
	EMU_DEFER(s, launch_adaptive_connections(c, depth, s));
	adaptive_connections_item(c, depth);
}
void launch_adaptive_reset(const AdaptiveView &a, stream_t s)
{
	EMU_DEFER(s, launch_adaptive_reset(a, s));
	for (uint32_t t = 0; t < a.count; t++)
		adaptive_reset_item(a, t);
}
void launch_adaptive_step(const AdaptiveView &a, uint32_t add, bool decide, stream_t s)
{
	EMU_DEFER(s, launch_adaptive_step(a, add, decide, s));
	for (uint32_t t = 0; t < a.count; t++)
		adaptive_step_item(a, add, decide, t);
}
void launch_present(const Params &p, f4 *out, float scale, int full, stream_t s)
{
	EMU_DEFER(s, launch_present(p, out, scale, full, s));
	for (uint32_t i = 0; i < p.fr.W * p.fr.local_rows; i++)
		present_item(p, out, scale, full, i);
}
void launch_deinterleave(const f4 *gathered, f4 *out, uint32_t W, uint32_t H, uint32_t local_rows, uint32_t world, stream_t s)
{
	EMU_DEFER(s, launch_deinterleave(gathered, out, W, H, local_rows, world, s));
	for (uint32_t i = 0; i < W * H; i++)
		deinterleave_item(gathered, out, W, H, local_rows, world, i);
}
void launch_denoise_guides(const Params &p, const DnView &d, f4 *surf, stream_t s, bool maps)
{
	EMU_DEFER(s, launch_denoise_guides(p, d, surf, s, maps));
	Ctx ctx(p);
	ctx.stk.overflow = d.overflow;
	for (uint32_t i = 0; i < d.W * d.H; i++)
		if (maps)
			dn_guide_maps_item(p, d, surf, i, ctx.stk);
		else if (surf)
			dn_guide_surf_item(p, d, surf, i, ctx.stk);
		else
			dn_guide_item(p, d, i, ctx.stk);
	for (uint32_t i = 0; i < d.W * d.H; i++)
		dn_gradient_item(d, i);
}
void launch_denoise_temporal(const DnView &d, const DnTemporal &t, const DnMotion *m, stream_t s)
{
	const DnMotion mv = m ? *m : DnMotion{}; // (a host record: taken at enqueue)
	const bool has_m = m != nullptr;
	EMU_DEFER(s, launch_denoise_temporal(d, t, has_m ? &mv : nullptr, s));
	for (uint32_t i = 0; i < d.W * d.H; i++)
		dn_demod_item(d, d.img[0], d.var[0], i);
	for (uint32_t i = 0; i < d.W * d.H; i++)
		if (m)
			dn_temporal_motion_item(d, t, *m, d.img[0], d.var[0], i);
		else
			dn_temporal_item(d, t, d.img[0], d.var[0], i);
}
void launch_denoise_filter(const DnView &d, const DnTemporal *t, const DnMotion *m, stream_t s)
{
	const DnTemporal tv = t ? *t : DnTemporal{}; // (host records: taken at enqueue)
	const DnMotion mv = m ? *m : DnMotion{};
	const bool has_t = t != nullptr, has_m = m != nullptr;
	EMU_DEFER(s, launch_denoise_filter(d, has_t ? &tv : nullptr, has_m ? &mv : nullptr, s));
	if (t)
		launch_denoise_temporal(d, *t, m, s);
	else
		for (uint32_t i = 0; i < d.W * d.H; i++)
			dn_demod_item(d, d.img[0], d.var[0], i);
	for (uint32_t k = 0; k < d.iterations; k++)
		for (uint32_t i = 0; i < d.W * d.H; i++)
			dn_pass_item(d, 1u << k, k + 1u == d.iterations, d.img[k & 1u], d.var[k & 1u], d.img[(k + 1u) & 1u], d.var[(k + 1u) & 1u], i);
}
// the direct fetch: texel(f4) is evaluated where the texel is read; item(fetch, x, y, alpha) = the kernel's item behind it
template <class Texel, class Item> static void display_loop(const DisplayView &v, const Texel &texel, const Item &item)
{
	const auto fetch = [&](int xi, int yi) -> f3 { return texel(v.in[(size_t)yi * v.W + (size_t)xi]); };
	for (uint32_t y = 0; y < v.H; y++)
		for (uint32_t x = 0; x < v.W; x++)
		{
			const float a = v.in[(size_t)y * v.W + x].w;
			item(fetch, (int)x, (int)y, a);
		}
}
void launch_display(const DisplayView &v, stream_t s)
{
	EMU_DEFER(s, launch_display(v, s));
	display_loop(
		v, [&](const f4 &c) -> f3 { return dp_tone(v, c); },
		[&](const auto &fetch, int x, int y, float a) { v.fxaa ? dp_item<true>(v, fetch, x, y, a) : dp_item<false>(v, fetch, x, y, a); });
}
void launch_display_exposed(const DisplayView &v, const ExposureView &e, stream_t s)
{
	EMU_DEFER(s, launch_display_exposed(v, e, s));
	const float E = e.rec->E;
	display_loop(
		v, [&](const f4 &c) -> f3 { return dp_tone(v, dp_exposed(c, E)); },
		[&](const auto &fetch, int x, int y, float a) { v.fxaa ? dp_item<true>(v, fetch, x, y, a) : dp_item<false>(v, fetch, x, y, a); });
}
// colour grading and dither (display_grade.h): the graded texel where it is read, dg_item behind it
void launch_display_graded(const DisplayView &v, const GradeView &g, stream_t s)
{
	EMU_DEFER(s, launch_display_graded(v, g, s));
	const float E = (g.flags & GR_EXPOSED) ? g.rec->E : 1.0f;
	display_loop(
		v, [&](const f4 &c) -> f3 { return dg_texel(v, g, c, E); },
		[&](const auto &fetch, int x, int y, float a) { v.fxaa ? dg_item<true>(v, g, fetch, x, y, a) : dg_item<false>(v, g, fetch, x, y, a); });
}
void launch_kat_grade(const GradeView &g, int which, const float *in, float *out, uint32_t n, stream_t s)
{
	EMU_DEFER(s, launch_kat_grade(g, which, in, out, n, s));
	for (uint32_t i = 0; i < n; i++)
		dg_kat_item(g, which, in, out, i);
}
// baseline JPEG (display_jpeg.h): the same items block by block; an interval's blocks are appended bit by bit, then stuffed
void launch_jpeg_blocks(const JpegView &v, stream_t s)
{
	EMU_DEFER(s, launch_jpeg_blocks(v, s));
	const uint32_t M = jp_mcu_size(v);
	uint32_t px[256];
	for (uint32_t m = 0; m < v.mcus; m++)
	{
		for (uint32_t y = 0; y < M; y++)
			for (uint32_t x = 0; x < M; x++)
				px[y * M + x] = jp_pixel(v, m, x, y);
		for (uint32_t k = 0; k < v.bpm; k++)
			jp_block_item(v, px, k, v.coef + ((size_t)m * v.bpm + k) * 64u);
	}
}
void launch_jpeg_entropy(const JpegView &v, stream_t s)
{
	EMU_DEFER(s, launch_jpeg_entropy(v, s));
	for (uint32_t i = 0; i < v.intervals; i++)
	{
		const uint32_t first = jp_interval_first(v, i), n = jp_interval_blocks(v, i);
		uint8_t *slot = v.slots + jp_slot(v, i);
		uint32_t out = 0u, stuffed = 0u, acc = 0u, have = 0u;
		const auto byte = [&](uint32_t b) {
			slot[out++] = (uint8_t)b;
			if (b == 255u)
				slot[out++] = 0u, stuffed++;
		};
		for (uint32_t b = first; b < first + n; b++)
		{
			uint32_t strip[JP_STRIP_WORDS];
			const uint32_t k = b % v.bpm, p = jp_prev_block(v.sub, b, first);
			const uint32_t len = jp_encode_block(*v.tab, v.coef + (size_t)b * 64u, p == ~0u ? 0 : (int)v.coef[(size_t)p * 64u],
												 v.sub ? (k >= 4u) : (k >= 1u), strip, 1u);
			for (uint32_t t = 0; t < len; t++)
			{
				acc = (acc << 1) | ((strip[t >> 5] >> (31u - (t & 31u))) & 1u);
				if (++have == 8u)
					byte(acc & 255u), acc = 0u, have = 0u;
			}
		}
		if (have)
			byte(((acc << (8u - have)) | ((1u << (8u - have)) - 1u)) & 255u);
		v.counts[2u * i] = out, v.counts[2u * i + 1u] = stuffed;
	}
}
void launch_jpeg_offsets(const JpegView &v, stream_t s)
{
	EMU_DEFER(s, launch_jpeg_offsets(v, s));
	uint64_t run = JP_HEADER;
	uint32_t stuffed = 0u;
	for (uint32_t i = 0; i < v.intervals; i++)
	{
		v.offsets[i] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
		run += (uint64_t)v.counts[2u * i] + 2u, stuffed += v.counts[2u * i + 1u];
	}
	jp_record(v, run, stuffed);
}
void launch_jpeg_pack(const JpegView &v, stream_t s)
{
	EMU_DEFER(s, launch_jpeg_pack(v, s));
	if (v.rec->overflow)
		return;
	for (uint32_t i = 0; i < v.intervals; i++)
	{
		const uint32_t n = v.counts[2u * i];
		uint8_t *dst = v.out + v.offsets[i];
		memcpy(dst, v.slots + jp_slot(v, i), n);
		dst[n] = 0xFFu, dst[n + 1u] = (uint8_t)jp_marker(v, i);
	}
}
// the exposure meter (metering.h): the same partial records, range by range, and the same fold
uint32_t meter_records(uint32_t pixels) { return (uint32_t)(((size_t)pixels + MT_RANGE - 1u) / MT_RANGE); }
void launch_meter_hist(const MeterView &v, stream_t s)
{
	EMU_DEFER(s, launch_meter_hist(v, s));
	for (uint32_t g = 0; g < meter_records(v.pixels); g++)
	{
		uint32_t *rec = v.partial + (size_t)g * MT_RECORD;
		for (uint32_t b = 0; b < MT_RECORD; b++)
			rec[b] = 0u;
		for (size_t i = (size_t)g * MT_RANGE; i < (size_t)(g + 1u) * MT_RANGE && i < v.pixels; i++)
		{
			const float Y = mt_luma(v.in[i]);
			rec[mt_valid(Y) ? mt_bin(Y) : MT_BINS]++;
		}
	}
}
void launch_meter_reduce(const uint32_t *partial, uint32_t records, uint32_t *hist, const MeterParams &m, MeterRecord *rec, stream_t s)
{
	EMU_DEFER(s, launch_meter_reduce(partial, records, hist, m, rec, s));
	for (uint32_t b = 0; b < MT_RECORD; b++)
	{
		uint32_t n = 0u;
		for (uint32_t r = 0; r < records; r++)
			n += partial[(size_t)r * MT_RECORD + b];
		hist[b] = n;
	}
	mt_finish(hist, hist[MT_BINS], m, rec);
}
// bloom (bloom.h): the same items texel by texel; a tap is fetched (and, in the first pass, staged) where the device reads LDS
uint32_t bloom_levels(uint32_t W, uint32_t H, uint32_t levels) { return bl_levels(W, H, levels); }
void launch_bloom_down0(const BloomDownView &v, const BloomParams &b, stream_t s)
{
	EMU_DEFER(s, launch_bloom_down0(v, b, s));
	const float E = *v.E;
	const auto fetch = [&](int x, int y) -> f4 { return bl_stage0(v.src[(size_t)dp_edge(y, (int)v.H) * v.W + (size_t)dp_edge(x, (int)v.W)], E, b); };
	for (uint32_t j = 0; j < v.Hn; j++)
		for (uint32_t i = 0; i < v.Wn; i++)
			v.dst[(size_t)j * v.Wn + i] = bl_down0_item(fetch, (int)i, (int)j);
}
void launch_bloom_down(const BloomDownView &v, stream_t s)
{
	EMU_DEFER(s, launch_bloom_down(v, s));
	const auto fetch = [&](int x, int y) -> f4 {
		const f4 t = v.src[(size_t)dp_edge(y, (int)v.H) * v.W + (size_t)dp_edge(x, (int)v.W)];
		return mk4(t.x, t.y, t.z, 0.0f);
	};
	for (uint32_t j = 0; j < v.Hn; j++)
		for (uint32_t i = 0; i < v.Wn; i++)
			v.dst[(size_t)j * v.Wn + i] = bl_down_item(fetch, (int)i, (int)j);
}
void launch_bloom_up(const BloomUpView &v, const BloomParams &b, stream_t s)
{
	EMU_DEFER(s, launch_bloom_up(v, b, s));
	for (size_t i = 0; i < (size_t)v.W * v.H; i++)
		bl_up_item(v, b.scatter, i);
}
void launch_bloom_apply(const BloomApplyView &v, const BloomParams &b, stream_t s)
{
	EMU_DEFER(s, launch_bloom_apply(v, b, s));
	for (size_t i = 0; i < (size_t)v.W * v.H; i++)
		bl_apply_item(v, b.intensity, i);
}
void launch_kat(const Params &p, const SkyView &sky, const LightTreeView &lt, int function, const float *in, float *out, uint32_t n, stream_t s)
{
	EMU_DEFER(s, launch_kat(p, sky, lt, function, in, out, n, s));
	float pot[POT_SLOTS];
	for (uint32_t i = 0; i < n; i++)
		if (function == KAT_METER_BIN)
			mt_kat_item(in, out, i);
		else if (function == KAT_SURFACE_MAPS)
			kat_maps_item(p, in, out, i);
		else
			kat_item<true>(p, sky, lt, function, in, out, i, pot);
}
void launch_skin_vertices(f4 *verts, f4 *vnormals, const f4 *base_verts, const f4 *base_normals, const uint32_t *joints4,
						  const f4 *weights4, const float *mats, uint32_t joint_count, uint32_t vertex_count, stream_t s)
{
	EMU_DEFER(s, launch_skin_vertices(verts, vnormals, base_verts, base_normals, joints4, weights4, mats, joint_count, vertex_count, s));
	for (uint32_t i = 0; i < vertex_count; i++)
		skin_vertex_item(verts, vnormals, base_verts, base_normals, joints4, weights4, mats, joint_count, i);
}
void launch_morph_vertices(f4 *verts, f4 *vnormals, const f4 *base_verts, const f4 *base_normals, const f4 *tgt_pos,
						   const f4 *tgt_nrm, const float *weights, uint32_t target_count, uint32_t vertex_count, stream_t s)
{
	EMU_DEFER(s, launch_morph_vertices(verts, vnormals, base_verts, base_normals, tgt_pos, tgt_nrm, weights, target_count, vertex_count, s));
	for (uint32_t i = 0; i < vertex_count; i++)
		morph_vertex_item(verts, vnormals, base_verts, base_normals, tgt_pos, tgt_nrm, weights, target_count, vertex_count, i);
}
void launch_skin_shade(TriShade *shade, const f4 *verts, const f4 *vnormals, const uint32_t *indices, uint32_t tri_count, stream_t s)
{
	EMU_DEFER(s, launch_skin_shade(shade, verts, vnormals, indices, tri_count, s));
	for (uint32_t i = 0; i < tri_count; i++)
		skin_shade_item(shade, verts, vnormals, indices, i);
}
void launch_stamp_instance(f4 *tri_verts, uint32_t tri_count, uint32_t instance, stream_t s)
{
	EMU_DEFER(s, launch_stamp_instance(tri_verts, tri_count, instance, s));
	for (uint32_t i = 0; i < tri_count; i++)
		tri_verts[3ull * i + 1].w = ubits(instance);
}
void launch_refresh4(Node4c *nodes4, const uint32_t *src4, uint32_t count4, const Node *blas_nodes2, stream_t s)
{
	EMU_DEFER(s, launch_refresh4(nodes4, src4, count4, blas_nodes2, s));
	for (uint32_t i = 0; i < count4; i++)
		refresh4_item(nodes4, src4, blas_nodes2, i);
}
void launch_expand4(const Node4c *nodes4, Node4f *out, uint32_t count4, stream_t s)
{
	EMU_DEFER(s, launch_expand4(nodes4, out, count4, s));
	for (uint32_t i = 0; i < count4; i++)
		expand4_item(nodes4, out, i);
}
uint32_t primary_entry_words() { return PRIMARY_ENTRY_K; }
void launch_primary_entry(const Node4f *nodes, uint32_t root, const CamView &cam, const FrameView &fr, uint32_t *out, uint32_t groups, stream_t s)
{
	EMU_DEFER(s, launch_primary_entry(nodes, root, cam, fr, out, groups, s));
	for (uint32_t i = 0; i < groups; i++)
	{
		uint32_t list[PRIMARY_ENTRY_K];
		primary_entry_item(nodes, root, cam, fr, i, out + (size_t)i * PRIMARY_ENTRY_K, list, 1u);
	}
}
void launch_order4f(const Node4f *in, Node4f *out, uint32_t first, uint32_t count, const float origin[3], bool ordered, stream_t s)
{
	const f3 c = mk3(origin[0], origin[1], origin[2]); // (a host array: taken at enqueue)
	const float cc[3] = {c.x, c.y, c.z};
	EMU_DEFER(s, launch_order4f(in, out, first, count, cc, ordered, s));
	for (uint32_t i = 0; i < count; i++)
		order4f_item(in, out, origin[0], origin[1], origin[2], ordered, first + i);
}
void launch_refit(Node *all_nodes, uint32_t node_base, const int *parents, uint32_t node_count, f4 *tri_verts,
				  uint32_t tri_base, const f4 *verts, const uint32_t *indices, uint32_t tri_count, uint32_t *flags, stream_t s)
{
	EMU_DEFER(s, launch_refit(all_nodes, node_base, parents, node_count, tri_verts, tri_base, verts, indices, tri_count, flags, s));
	for (uint32_t i = 0; i < tri_count; i++)
		refit_tris_item(tri_verts + 3ull * tri_base, verts, indices, i);
	memset(flags, 0, sizeof(uint32_t) * node_count);
	Node *nodes = all_nodes + node_base;
	for (uint32_t i = 0; i < node_count; i++)
	{
		const Node n = nodes[i];
		if (n.count < 0 || i == 1u)
			continue;
		float mn[3], mx[3];
		leaf_bounds(n, tri_verts, mn, mx);
		for (int a = 0; a < 3; a++)
			nodes[i].bmin[a] = mn[a], nodes[i].bmax[a] = mx[a];
		int cur = (int)i;
		for (;;)
		{
			const int parent = parents[cur];
			if (parent < 0)
				break;
			if (flags[parent]++ == 0u)
				break;
			const int l = (int)(((uint32_t)nodes[parent].left_first & ENTRY_INDEX_MASK) - node_base);
			for (int a = 0; a < 3; a++)
			{
				nodes[parent].bmin[a] = fminf(nodes[l].bmin[a], nodes[l + 1].bmin[a]);
				nodes[parent].bmax[a] = fmaxf(nodes[l].bmax[a], nodes[l + 1].bmax[a]);
			}
			cur = parent;
		}
	}
}

void launch_light_refresh(const LightFollowView &v, stream_t s)
{
	EMU_DEFER(s, launch_light_refresh(v, s));
	for (uint32_t i = 0; i < v.n_area; i++)
		*v.bound_count += lf_refresh_item(v, i) ? 1u : 0u;
}
void launch_light_tree_refit(LightTreeNode *nodes, const LightTreeLevels &lv, const AreaLight *area, uint32_t n_area,
							 const unsigned char *bound, unsigned char *touched, stream_t s)
{
	EMU_DEFER(s, launch_light_tree_refit(nodes, lv, area, n_area, bound, touched, s));
	for (uint32_t l = lv.levels; l-- > 0u;)
		for (uint32_t i = 0; i < lv.count[l]; i++)
			lf_refit_item(nodes, area, n_area, bound, touched, lv.first[l] + i);
}
