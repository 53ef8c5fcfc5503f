// light_tree.h — the host side of light_sampling=tree: the binary tree over the area, point and spot lights that the light-tree
// variant of the shade kernel descends (rt_core.h: lt_importance / lt_sample / lt_pick_prob; formulas: include/rfwhip.h,
// DESIGN.md section 12).  Directional lights have no position: they stay a flat list beside the root.
//
// Built top-down in double: the lights of a node are ordered by (centroid along the longest axis of the centroid box, light index)
// and split at the median, the left side taking the odd one — coincident lights terminate, the depth is ceil(log2 n).  A leaf holds
// one light.  A node's box bounds the lights below it (all three vertices of a triangle), its energy is the sum of theirs, its cone
// bounds their normals (Conty Estevez and Kulla 2018, Alg. 1); a point or spot light emits in every direction as far as the tree
// is concerned (cos_o = -1), which is conservative for a spot.  Header-only: rfwhip_api.cpp is its one user.
#pragma once
#include "rt_types.h"
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// Every build of this header gives the same tree to the bit: no contraction of a * b + c into fma (the product is compiled by
// clang, the tests' emulation by g++ with -mfma).  The g++ pragma applies to the functions defined between push and pop — the
// two of this header — and pop restores the options of the including file (rfwhip_api.cpp, its one user): nothing outside the
// header is compiled differently, and both functions are called once per tree, so what the option costs in inlining is nothing.
#if defined(__clang__)
#define LT_FP_STRICT _Pragma("clang fp contract(off)")
#else
#define LT_FP_STRICT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

namespace lighttree
{
struct Cone
{
	double axis[3];
	double theta_o; // half angle; pi: every direction
};
struct Item
{
	uint32_t light;
	double c[3], lo[3], hi[3], energy;
	Cone cone;
};
constexpr double PI = 3.14159265358979323846;

inline double energy_of(float e) { return e > 0.0f ? (double)e : 0.0; } // (negative or NaN: 0)

inline Cone cone_union(Cone a, Cone b)
{
	LT_FP_STRICT
	if (b.theta_o > a.theta_o)
		std::swap(a, b);
	if (a.theta_o >= PI)
		return a;
	const double d = std::min(1.0, std::max(-1.0, a.axis[0] * b.axis[0] + a.axis[1] * b.axis[1] + a.axis[2] * b.axis[2]));
	const double theta_d = std::acos(d);
	if (std::min(theta_d + b.theta_o, PI) <= a.theta_o)
		return a;
	Cone r = a;
	r.theta_o = 0.5 * (a.theta_o + theta_d + b.theta_o);
	if (r.theta_o >= PI)
	{
		r.theta_o = PI;
		return r;
	}
	// a's axis turned by theta_r towards b's, about a x b (Rodrigues; the axis of rotation is perpendicular to a's)
	const double theta_r = r.theta_o - a.theta_o;
	double k[3] = {a.axis[1] * b.axis[2] - a.axis[2] * b.axis[1], a.axis[2] * b.axis[0] - a.axis[0] * b.axis[2],
				   a.axis[0] * b.axis[1] - a.axis[1] * b.axis[0]};
	const double kl = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
	if (!(kl > 1e-12)) // (opposite axes: no plane to turn in)
	{
		r.theta_o = PI;
		return r;
	}
	for (double &x : k)
		x /= kl;
	const double kxa[3] = {k[1] * a.axis[2] - k[2] * a.axis[1], k[2] * a.axis[0] - k[0] * a.axis[2], k[0] * a.axis[1] - k[1] * a.axis[0]};
	const double cs = std::cos(theta_r), sn = std::sin(theta_r);
	double l = 0.0;
	for (int i = 0; i < 3; i++)
		r.axis[i] = a.axis[i] * cs + kxa[i] * sn, l += r.axis[i] * r.axis[i];
	l = std::sqrt(l);
	for (double &x : r.axis)
		x /= l;
	return r;
}

// The tree of the given lights.  nodes: empty without a spatial light, one node for one light, 2 n nodes for n >= 2 (node 1 unused).
// paths: one entry per light of all four kinds, in pot_any()'s order.
inline void build(const rt::AreaLight *area, uint32_t n_area, const rt::PointLight *point, uint32_t n_point, const rt::SpotLight *spot,
				  uint32_t n_spot, uint32_t n_dir, std::vector<rt::LightTreeNode> &nodes, std::vector<rt::LightTreePath> &paths)
{
	LT_FP_STRICT
	const uint32_t n = n_area + n_point + n_spot;
	nodes.clear();
	paths.assign((size_t)n + n_dir, rt::LightTreePath{0u, 0u});
	if (!n)
		return;
	std::vector<Item> items(n);
	for (uint32_t i = 0; i < n; i++)
	{
		Item &it = items[i];
		it.light = i;
		if (i < n_area)
		{
			const rt::AreaLight &l = area[i];
			const float *v[3] = {l.vertex0, l.vertex1, l.vertex2};
			for (int a = 0; a < 3; a++)
			{
				it.c[a] = ((double)v[0][a] + (double)v[1][a] + (double)v[2][a]) / 3.0;
				it.lo[a] = std::min({(double)v[0][a], (double)v[1][a], (double)v[2][a]});
				it.hi[a] = std::max({(double)v[0][a], (double)v[1][a], (double)v[2][a]});
			}
			it.energy = energy_of(l.energy);
			const double nl = std::sqrt((double)l.normal[0] * l.normal[0] + (double)l.normal[1] * l.normal[1] + (double)l.normal[2] * l.normal[2]);
			if (nl > 0.0 && std::isfinite(nl))
				it.cone = Cone{{l.normal[0] / nl, l.normal[1] / nl, l.normal[2] / nl}, 0.0};
			else
				it.cone = Cone{{0, 0, 1}, PI};
		}
		else
		{
			const float *p = i < n_area + n_point ? point[i - n_area].position : spot[i - n_area - n_point].position;
			for (int a = 0; a < 3; a++)
				it.c[a] = it.lo[a] = it.hi[a] = (double)p[a];
			it.energy = energy_of(i < n_area + n_point ? point[i - n_area].energy : spot[i - n_area - n_point].energy);
			it.cone = Cone{{0, 0, 1}, PI};
		}
	}
	nodes.assign(n == 1 ? 1 : 2 * (size_t)n, rt::LightTreeNode{});
	struct Job
	{
		uint32_t node, first, count, bits, depth;
	};
	std::vector<Job> jobs{{0u, 0u, n, 0u, 0u}};
	uint32_t next = 2; // the next free sibling pair
	// (breadth first: the nodes of a level sit together)
	for (size_t j = 0; j < jobs.size(); j++)
	{
		const Job job = jobs[j];
		Item *const first = items.data() + job.first;
		rt::LightTreeNode &nd = nodes[job.node];
		double lo[3], hi[3], clo[3], chi[3], e = 0.0;
		Cone cone = first[0].cone;
		for (int a = 0; a < 3; a++)
			lo[a] = first[0].lo[a], hi[a] = first[0].hi[a], clo[a] = chi[a] = first[0].c[a];
		for (uint32_t i = 0; i < job.count; i++)
		{
			for (int a = 0; a < 3; a++)
			{
				lo[a] = std::min(lo[a], first[i].lo[a]), hi[a] = std::max(hi[a], first[i].hi[a]);
				clo[a] = std::min(clo[a], first[i].c[a]), chi[a] = std::max(chi[a], first[i].c[a]);
			}
			e += first[i].energy;
			if (i)
				cone = cone_union(cone, first[i].cone);
		}
		for (int a = 0; a < 3; a++)
		{
			// (rounded outwards: the float box contains the double one)
			nd.lo[a] = (float)lo[a], nd.hi[a] = (float)hi[a];
			if ((double)nd.lo[a] > lo[a])
				nd.lo[a] = std::nextafterf(nd.lo[a], -INFINITY);
			if ((double)nd.hi[a] < hi[a])
				nd.hi[a] = std::nextafterf(nd.hi[a], INFINITY);
			nd.axis[a] = (float)cone.axis[a];
		}
		nd.energy = (float)e;
		// (rounded towards -1: the float cone contains the double one)
		const double co = cone.theta_o >= PI ? -1.0 : std::cos(cone.theta_o);
		nd.cos_o = (float)co;
		if ((double)nd.cos_o > co)
			nd.cos_o = std::nextafterf(nd.cos_o, -2.0f);
		nd.count = job.count;
		if (job.count == 1)
		{
			nd.child = 0u, nd.light = first[0].light;
			paths[first[0].light] = rt::LightTreePath{job.bits, job.depth};
			continue;
		}
		int ax = 0;
		if (chi[1] - clo[1] > chi[ax] - clo[ax])
			ax = 1;
		if (chi[2] - clo[2] > chi[ax] - clo[ax])
			ax = 2;
		// (a NaN centroid — a light with a NaN position — sorts last, by index: the comparison stays a strict weak order)
		std::sort(first, first + job.count, [ax](const Item &a, const Item &b) {
			const double ka = a.c[ax] == a.c[ax] ? a.c[ax] : INFINITY, kb = b.c[ax] == b.c[ax] ? b.c[ax] : INFINITY;
			return ka < kb || (ka == kb && a.light < b.light);
		});
		const uint32_t nl = (job.count + 1u) / 2u;
		nd.child = next, nd.light = 0u;
		jobs.push_back({next, job.first, nl, job.bits, job.depth + 1u});
		jobs.push_back({next + 1u, job.first + nl, job.count - nl, job.bits | (1u << job.depth), job.depth + 1u});
		next += 2u;
	}
}

// The level ranges of a tree in build()'s layout, for the refit on the device (light_follow.h): level l is the nodes
// [first[l], first[l] + count[l]), level 0 the root, level 1 starts at node 2, every further level directly behind the one above.
// Checked on the way, because the refit indexes by what the nodes say: a child pair is even, inside the table and behind its
// parent's level, a leaf's light is one of the n_spatial lights, the table has build()'s size.  false: not such a tree.
inline bool levels(const rt::LightTreeNode *nodes, size_t node_count, uint32_t n_spatial, uint32_t *first, uint32_t *count, uint32_t max_levels,
				   uint32_t &n_levels)
{
	n_levels = 0;
	if (!node_count)
		return n_spatial == 0;
	if (node_count != (n_spatial == 1 ? (size_t)1 : 2 * (size_t)n_spatial) || !max_levels)
		return false;
	first[0] = 0u, count[0] = 1u, n_levels = 1;
	for (;;)
	{
		const uint32_t l = n_levels - 1u, end = l ? first[l] + count[l] : 2u;
		uint32_t lo = 0xFFFFFFFFu, hi = 0u, inner = 0u;
		for (uint32_t i = first[l]; i < first[l] + count[l]; i++)
		{
			const rt::LightTreeNode &nd = nodes[i];
			if (!nd.child)
			{
				if (nd.light >= n_spatial)
					return false;
				continue;
			}
			if ((nd.child & 1u) || nd.child < end || (size_t)nd.child + 1u >= node_count)
				return false;
			lo = std::min(lo, nd.child), hi = std::max(hi, nd.child + 2u), inner++;
		}
		if (!inner)
			break;
		if (lo != end || hi - lo != 2u * inner || n_levels == max_levels)
			return false;
		first[n_levels] = lo, count[n_levels] = hi - lo, n_levels++;
	}
	return node_count == 1 || (size_t)first[n_levels - 1u] + count[n_levels - 1u] == node_count;
}
} // namespace lighttree
#if !defined(__clang__)
#pragma GCC pop_options
#endif
#undef LT_FP_STRICT
