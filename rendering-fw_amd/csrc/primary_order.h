// primary_order.h — the work item of the primary wave's node ORDERING pass.  Included by kernels.hip inside
// namespace rtk, behind expand4_item: the device kernel (k_order4f) and the host emulation (kernels_emu.inc) run the same item.
//
// Every primary ray of a call leaves from the camera position (or from a lens disc around it), so the near-to-far order of a node's
// children is almost a function of the node and the camera alone.  The pass writes, for an origin C, a SECOND float node table
// (same size, same indexing as SceneView::nodes4f: an entry names the same node in both) whose nodes hold the same four children
// PERMUTED near to far as seen from C; the packet form of the primary wave then takes the children as they come (trace_packet,
// ORDERED) instead of sorting them per wave and node step on the scalar unit.
//   key of a child, ascending:  d2 = squared distance from C to the child's box (0 inside the box)
//                               then the squared distance from C to the box centre
//                               then the original slot
//   An unused slot (ENTRY_EMPTY, or a box inverted on some axis) goes last and stays as it is: inverted, never entered.
//   A child's six planes and its entry move together; nothing else of the node changes.
// Child order never decides which hit a closest-hit ray reports (tri_test<TIE>: the hit is a function of ray and scene), so ANY
// order — of another camera, of another space, none at all — gives the same image; only the number of nodes walked depends on it.
#pragma once

// distance from c to the interval [lo, hi] on one axis (0 inside)
RT_FN float po_axis_d(float lo, float hi, float c) { return fmaxf(fmaxf(lo - c, c - hi), 0.0f); }

// one child with its key
struct PoChild
{
	float lo[3], hi[3];
	uint32_t entry, pad;
	float d2, dc2;
	bool empty;
};
// does b come before a?  (strictly: equal keys keep their slots)
RT_FN bool po_before(const PoChild &b, const PoChild &a)
{
	if (a.empty != b.empty)
		return a.empty;
	return !a.empty && (b.d2 < a.d2 || (b.d2 == a.d2 && b.dc2 < a.dc2));
}

// node i of `in`, its children ordered as seen from (cx, cy, cz), into node i of `out` (another table: never in place).
// ordered = false: the node is copied as it is (a mesh tree several instances share has no one object-space camera position)
RT_FN void order4f_item(const Node4f *in, Node4f *out, float cx, float cy, float cz, bool ordered, uint32_t i)
{
	const Node4f n = in[i];
	if (!ordered)
	{
		out[i] = n;
		return;
	}
	const float c[3] = {cx, cy, cz};
	PoChild ch[4];
#pragma unroll
	for (int k = 0; k < 4; k++)
	{
		PoChild &q = ch[k];
		q.entry = n.entry[k], q.pad = n.pad[k];
		q.empty = q.entry == ENTRY_EMPTY;
		q.d2 = 0.0f, q.dc2 = 0.0f;
#pragma unroll
		for (int a = 0; a < 3; a++)
		{
			q.lo[a] = n.lo[a][k], q.hi[a] = n.hi[a][k];
			q.empty = q.empty || q.lo[a] > q.hi[a];
			const float d = po_axis_d(q.lo[a], q.hi[a], c[a]), dc = (q.lo[a] + q.hi[a]) * 0.5f - c[a];
			q.d2 += d * d, q.dc2 += dc * dc;
		}
	}
	// insertion sort by neighbour swaps, every index a constant (the children stay in registers); stable
#pragma unroll
	for (int j = 1; j < 4; j++)
#pragma unroll
		for (int q = j; q > 0; q--)
			if (po_before(ch[q], ch[q - 1]))
			{
				const PoChild t = ch[q - 1];
				ch[q - 1] = ch[q], ch[q] = t;
			}
	Node4f f;
#pragma unroll
	for (int k = 0; k < 4; k++)
	{
#pragma unroll
		for (int a = 0; a < 3; a++)
			f.lo[a][k] = ch[k].lo[a], f.hi[a][k] = ch[k].hi[a];
		f.entry[k] = ch[k].entry, f.pad[k] = ch[k].pad;
	}
	out[i] = f;
}
