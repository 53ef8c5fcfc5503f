// skyhdr_san_main.cpp — the host-callable half of csrc/sky_load.h (the header walk and the work items, run serially over plain heap
// arrays of exactly the size the library gives them) under the host sanitizers.  tests/test_sky_load.py compiles this file with
// -fsanitize=address,undefined and runs it as a child process over the malformed files and the model's files: every file must come
// back with a line "<path> <code> <plane flags>", the table's chain over a few weight vectors with "tables ok", and the process
// must exit 0 (a sanitizer report ends it with another status).
#include "sky_load.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace rtk;

static int one(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f)
	{
		fprintf(stderr, "cannot open %s\n", path);
		return 2;
	}
	std::vector<uint8_t> in;
	uint8_t buf[4096];
	for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;)
		in.insert(in.end(), buf, buf + n);
	fclose(f);
	// (a heap copy of exactly the file's size: a read past its end is a report)
	uint8_t *stream = (uint8_t *)malloc(in.size() ? in.size() : 1);
	memcpy(stream, in.data(), in.size());
	SkyHdrInfo info;
	const int rc = skyhdr_walk(stream, in.size(), info);
	uint32_t errors = 0u;
	if (rc == SKY_OK)
		for (const uint32_t m : {0u, SKY_FLIP_ROWS})
		{
			SkyHdrView v;
			memset(&v, 0, sizeof(v));
			const size_t items = (size_t)info.H * 4u;
			std::vector<uint8_t> planes(info.rle_lines ? items * info.W : 0u);
			std::vector<uint32_t> flags(items);
			SkyF4 *out = (SkyF4 *)aligned_alloc(16, (size_t)info.W * info.H * sizeof(SkyF4));
			v.stream = stream, v.ranges = info.ranges.data(), v.planes = planes.empty() ? nullptr : planes.data(), v.flags = flags.data();
			v.out = out, v.W = info.W, v.H = info.H, v.mods = m;
			if (info.rle_lines)
				skyhdr_host_planes(v);
			skyhdr_host_texels(v);
			for (const uint32_t w : flags)
				errors |= w;
			free(out);
		}
	printf("%s %d %u %s\n", path, rc, errors, rc ? info.msg : "");
	free(stream);
	return 0;
}

// skyhdr_plane over strings the walk refuses, with hand-made offsets (the item must flag them whoever hands it the ranges): a plane
// of W = 8 bytes from exactly-sized heap arrays -> the item's flags
static uint32_t plane_flags(const std::vector<uint8_t> &bytes)
{
	uint8_t *stream = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
	memcpy(stream, bytes.data(), bytes.size());
	const uint32_t end = (uint32_t)bytes.size();
	const uint32_t ranges[5] = {0u, end, end, end, end}; // component 0 owns the string, the others are empty
	std::vector<uint8_t> planes(4u * 8u, 0xEEu);
	std::vector<uint32_t> flags(4u);
	SkyHdrView v;
	memset(&v, 0, sizeof(v));
	v.stream = stream, v.ranges = ranges, v.planes = planes.data(), v.flags = flags.data(), v.W = 8u, v.H = 1u;
	skyhdr_host_planes(v);
	free(stream);
	for (uint32_t c = 1; c < 4u; c++)
		if (flags[c] != SKY_ERR_TRUNCATED) // (an empty string ends early)
			exit(6);
	return flags[0];
}

// the table's chain over n weights, every array of exactly its size -> the record's flags
static uint32_t table(uint32_t n, int kind)
{
	const uint32_t nb1 = skytab_blocks(n), nb2 = skytab_blocks(nb1);
	std::vector<double> w(n), D(n), E(n), t1d(nb1), t1e(nb1), t2d(nb2), t2e(nb2);
	std::vector<SkyPartial> part(nb1);
	std::vector<uint32_t> c1(nb1), c2(nb2);
	std::vector<SkyAliasEntry> out(n);
	uint32_t x = 12345u + n;
	for (uint32_t k = 0; k < n; k++)
	{
		x = x * 1664525u + 1013904223u;
		w[k] = kind == 0 ? 0.25 : kind == 1 ? (k && (x >> 8) % 10u < 7u ? 0.0 : (double)(x >> 8)) : kind == 2 ? (k == n / 2u ? 1e9 : 1e-3) : 0.0;
	}
	SkyTabRecord rec;
	SkyTabView v;
	memset(&v, 0, sizeof(v));
	v.w = w.data(), v.D = D.data(), v.E = E.data(), v.part = part.data(), v.t1d = t1d.data(), v.t1e = t1e.data(), v.t2d = t2d.data(), v.t2e = t2e.data();
	v.c1 = c1.data(), v.c2 = c2.data(), v.rec = &rec, v.table = out.data(), v.W = 1u, v.n = n, v.nb1 = nb1, v.nb2 = nb2;
	skytab_host_weights(v), skytab_host_total(v), skytab_host_scan_block(v), skytab_host_scan_super(v), skytab_host_scan_top(v);
	skytab_host_scan_apply(v), skytab_host_assign(v);
	for (uint32_t k = 0; k < n; k++)
		if (out[k].alias >= n || !(out[k].keep >= 0.0f && out[k].keep <= 1.0f))
			exit(4);
	for (uint32_t k = 1; k < n; k++)
		if (D[k] < D[k - 1u] || E[k] < E[k - 1u]) // the prefix sums are non-decreasing
			exit(5);
	return rec.flags;
}

int main(int argc, char **argv)
{
	for (int i = 1; i < argc; i++)
		if (one(argv[i]))
			return 2;
	for (const uint32_t n : {1u, 2u, SKYTAB_B - 1u, SKYTAB_B, SKYTAB_B + 1u, 2u * SKYTAB_B + 1u, SKYTAB_B * SKYTAB_B + 1u})
		for (int kind = 0; kind < 4; kind++)
			if (((table(n, kind) & SKYTAB_VALID) != 0u) != (kind != 3))
				return 3;
	if (plane_flags({136, 7}) != 0u || plane_flags({131, 9, 0, 133, 9}) != SKY_ERR_ZERO || plane_flags({133, 9, 133, 9}) != SKY_ERR_OVERRUN ||
		plane_flags({5, 1, 2, 3, 4, 5, 5, 1, 2, 3, 4, 5}) != SKY_ERR_OVERRUN || plane_flags({136}) != SKY_ERR_TRUNCATED ||
		plane_flags({8, 1, 2, 3}) != SKY_ERR_TRUNCATED || plane_flags({131, 9}) != SKY_ERR_TRUNCATED)
		return 7;
	printf("tables ok\n");
	return 0;
}
