// texdec_san_main.cpp — the host-callable half of csrc/texture_decode.h (the marker walk and the work items, run serially over plain
// heap arrays of exactly the size the library gives them) under the host sanitizers.  tests/test_texture_decode.py compiles this file
// with -fsanitize=address,undefined and runs it as a child process over the malformed streams and the golden streams: every file must
// come back with a line "<code> <error flags>" and the process must exit 0 (a sanitizer report ends it with another status).
#include "texture_decode.h"

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
	// (a heap copy of exactly the stream's size: a read past its end is a report)
	uint8_t *stream = (uint8_t *)malloc(in.size() ? in.size() : 1);
	memcpy(stream, in.data(), in.size());
	TdInfo info;
	const int rc = td_walk(stream, in.size(), info);
	uint32_t errors = 0u;
	if (rc == TD_OK)
		for (const uint32_t m : {0u, TD_FLIP_ROWS | TD_LINEARIZE_REFERENCE, TD_FLIP_ROWS | TD_LINEARIZE_SRGB})
		{
			TexdecView v;
			memset(&v, 0, sizeof(v));
			size_t planes = 0;
			td_view_geometry(info, v, &planes);
			std::vector<int16_t> coef((size_t)v.blocks * 64u);
			std::vector<uint32_t> flags(v.intervals), alpha(td_tiles(v.W, v.H)), out(td_chain_texels(v.W, v.H));
			std::vector<uint8_t> pl(planes);
			uint8_t lin[256];
			td_srgb_table(lin);
			TexRecord rec;
			v.stream = stream, v.ranges = info.ranges.data(), v.tab = &info.tab, v.coef = coef.data(), v.flags = flags.data();
			v.planes = pl.data(), v.out = out.data(), v.lin = lin, v.rec = &rec, v.alpha = alpha.data(), v.mods = m;
			v.tiles = td_tiles(v.W, v.H), v.path = TD_PATH_HOST;
			td_host_zero(v);
			td_host_entropy(v);
			td_host_idct(v);
			td_host_color(v);
			td_host_mips(v);
			td_host_finish(v);
			errors |= rec.errors;
		}
	printf("%s %d %u %s\n", path, rc, errors, rc ? info.msg : "");
	free(stream);
	return 0;
}

int main(int argc, char **argv)
{
	for (int i = 1; i < argc; i++)
		if (one(argv[i]))
			return 2;
	// PNG's filters over rows of exactly their size
	for (int type = 0; type <= 4; type++)
	{
		const size_t rows = 5, row_bytes = 13, bpp = 3;
		std::vector<uint8_t> in(rows * (row_bytes + 1)), out(rows * row_bytes);
		for (size_t i = 0; i < in.size(); i++)
			in[i] = (uint8_t)(i * 37u + 11u);
		for (size_t y = 0; y < rows; y++)
			in[y * (row_bytes + 1)] = (uint8_t)type;
		if (td_png_unfilter(in.data(), rows, row_bytes, bpp, out.data()) != TD_OK)
			return 3;
	}
	return 0;
}
