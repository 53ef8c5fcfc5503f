// bloom_host.cpp — bloom through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY (and RFWHIP_BLOOM, when the test sets
// it) in the environment, drive the rfw::RenderContext through its virtual interface for one frame and write what hiprtReadDisplay
// returns to <out>/plugin.rgba8.  Beside it, from a group driven through the C ABI directly on the same scene WITHOUT any
// display_bloom* setting touched: the linear image of the same frame (<out>/abi.f32, W x H float4) and its display bytes
// (<out>/abi.rgba8).  tests/test_bloom_plugin_gpu.py holds the plugin's bytes to the float64 models on abi.f32 (RFWHIP_BLOOM=1) or
// to abi.rgba8 (unset).  The plugin is created FIRST: a value of RFWHIP_BLOOM it refuses ends the program (exit status 5, the
// message on stderr) before anything renders.
#include "host_common.h"

// the C ABI's frame 0 without bloom: the linear image and its display bytes
static int reference(const SceneData &s, const char *tonemap, const std::string &out)
{
	rfwhip_group *g = nullptr;
	if (int r = reference_group(&g))
		return r;
	ABI(rfwhip_group_set_setting(g, "display_tonemap", tonemap));
	if (int r = upload_abi(g, s))
		return r;
	const rfwhip_camera cam = pod(camera());
	std::vector<float> linear(size_t(W) * H * 4);
	std::vector<uint8_t> bytes(size_t(W) * H * 4);
	ABI(rfwhip_group_render(g, &cam, RFWHIP_RESET));
	ABI(rfwhip_group_read_framebuffer(g, linear.data()));
	ABI(rfwhip_group_read_display(g, RFWHIP_DISPLAY_RGBA8, bytes.data()));
	rfwhip_group_destroy(g);
	if (int r = dump(out + "/abi.f32", linear.data(), linear.size() * sizeof(float)))
		return r;
	return dump(out + "/abi.rgba8", bytes.data(), bytes.size());
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".", out = argc > 2 ? argv[2] : ".";
	const char *tonemap = std::getenv("RFWHIP_DISPLAY") ? std::getenv("RFWHIP_DISPLAY") : "aces";
	SceneData s(glm::vec3{2.0f, 4.0f, 8.0f});
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadDisplay"}))
		return r;
	auto read_display = (ReadDisplayFn)p.sym[0];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		if (int r = reference(s, tonemap, out))
			return r;
		upload(ctx, s);
		std::vector<uint8_t> img(size_t(W) * H * 4);
		ctx->render_frame(camera(), rfw::Reset);
		if (read_display(ctx, img.data()) != 0)
			rc = 4;
		if (int r = dump(out + "/plugin.rgba8", img.data(), img.size()))
			rc = r;
		std::printf("size %u %u\n", W, H);
		return 0;
	});
}
