// jpeg_host.cpp — the JPEG of the presented frame through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY and the
// RFWHIP_JPEG_* variables the test sets in the environment, drive the rfw::RenderContext through its virtual interface for one frame
// and write what hiprtReadDisplay returns to <out>/plugin.rgba8 and what hiprtReadJpeg returns to <out>/plugin.jpg.
// tests/test_jpeg_plugin_gpu.py encodes plugin.rgba8 with the numpy model under the same settings and asks for equal bytes.  A value
// the plugin refuses ends the program (exit status 5, the message on stderr) before anything renders.  A second hiprtReadJpeg with
// a cap one byte short must fail, name the length and leave its buffer alone (exit status 8 otherwise).
#include "host_common.h"

typedef int (*JpegFn)(rfw::RenderContext *, void *, size_t, size_t *);
typedef int (*BoundFn)(rfw::RenderContext *, size_t *);

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".", out = argc > 2 ? argv[2] : ".";
	SceneData s(glm::vec3{2.0f, 4.0f, 8.0f});
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadDisplay", "hiprtReadJpeg", "hiprtJpegBound"}))
		return r;
	auto read_display = (ReadDisplayFn)p.sym[0];
	auto read_jpeg = (JpegFn)p.sym[1];
	auto jpeg_bound = (BoundFn)p.sym[2];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		upload(ctx, s);
		std::vector<uint8_t> img(size_t(W) * H * 4);
		ctx->render_frame(camera(), rfw::Reset);
		if (read_display(ctx, img.data()) != 0)
			rc = 4;
		if (int r = dump(out + "/plugin.rgba8", img.data(), img.size()))
			rc = r;
		size_t bound = 0, bytes = 0, needed = 0;
		if (jpeg_bound(ctx, &bound) != 0)
			rc = 4;
		std::vector<uint8_t> jpg(bound), small(bound, 0xA5);
		if (read_jpeg(ctx, jpg.data(), jpg.size(), &bytes) != 0 || bytes > bound)
			rc = 4;
		else if (int r = dump(out + "/plugin.jpg", jpg.data(), bytes))
			rc = r;
		if (!rc && (read_jpeg(ctx, small.data(), bytes - 1, &needed) == 0 || needed != bytes || small[0] != 0xA5 || small[bytes - 1] != 0xA5))
			rc = 8;
		std::printf("size %u %u bound %zu bytes %zu\n", W, H, bound, bytes);
		return 0;
	});
}
