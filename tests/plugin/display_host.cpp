// display_host.cpp — the display stage through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY set in the environment,
// drive the rfw::RenderContext through its virtual interface, and compare the bytes hiprtReadDisplay returns after every
// render_frame (RFWHIP_FRAMES_IN_FLIGHT of the environment: frame k - n + 1) with the bytes rfwhip_group_read_display gives for the
// same frames of a group driven through the C ABI directly, on the same scene with the same display_tonemap.  The reference group
// renders BEFORE the plugin is opened.
#include "host_common.h"

static const int FRAMES = 5;

// the C ABI's display images (RGBA8) of frames 0 .. FRAMES - 1, and the float image of the last one
static int reference(const SceneData &s, const char *tonemap, std::vector<std::vector<uint8_t>> &want, std::vector<float> &raw)
{
	rfwhip_group *g = nullptr;
	if (int r = reference_group(&g))
		return r;
	ABI(rfwhip_group_set_setting(g, "display_tonemap", tonemap));
	if (int r = upload_abi(g, s))
		return r;
	const rfwhip_camera cam = pod(camera());
	want.assign(FRAMES, std::vector<uint8_t>(size_t(W) * H * 4));
	for (int k = 0; k < FRAMES; k++)
	{
		ABI(rfwhip_group_render(g, &cam, k == 0 ? RFWHIP_RESET : RFWHIP_CONVERGE));
		ABI(rfwhip_group_read_display(g, RFWHIP_DISPLAY_RGBA8, want[(size_t)k].data()));
	}
	raw.assign(size_t(W) * H * 4, 0.0f);
	ABI(rfwhip_group_read_framebuffer(g, raw.data()));
	rfwhip_group_destroy(g);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const int in_flight = std::getenv("RFWHIP_FRAMES_IN_FLIGHT") ? std::max(1, std::atoi(std::getenv("RFWHIP_FRAMES_IN_FLIGHT"))) : 1;
	const char *tonemap = std::getenv("RFWHIP_DISPLAY") ? std::getenv("RFWHIP_DISPLAY") : "aces";
	SceneData s(glm::vec3{0.25f, 0.5f, 0.75f});
	std::vector<std::vector<uint8_t>> want;
	std::vector<float> raw;
	if (int rc = reference(s, tonemap, want, raw))
		return rc;
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadDisplay"}))
		return r;
	auto read_display = (ReadDisplayFn)p.sym[0];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		upload(ctx, s);
		const rfw::Camera cam = camera();
		std::vector<uint8_t> img(size_t(W) * H * 4);
		int equal = 0;
		for (int k = 0; k < FRAMES; k++)
		{
			ctx->render_frame(cam, k == 0 ? rfw::Reset : rfw::Converge);
			if (read_display(ctx, img.data()) != 0)
				rc = 4;
			// what render_frame hands out with n frames in flight: frame k - n + 1 (frame 0 until there is an older one)
			const int shown = std::max(0, k - in_flight + 1);
			equal += std::memcmp(img.data(), want[(size_t)shown].data(), img.size()) == 0;
		}
		std::printf("frames %d equal %d\n", FRAMES, equal);
		// the bytes are a display image: the colour varies over the image, and alpha is the float image's, clamped and quantised
		int distinct = 0, opaque = 0;
		for (size_t i = 0; i < size_t(W) * H; i++)
		{
			distinct += want.back()[4 * i] != want.back()[4 * (i ? i - 1 : 0)];
			opaque += want.back()[4 * i + 3] == (uint8_t)std::lrint(std::fmin(std::fmax(raw[4 * i + 3], 0.0f), 1.0f) * 255.0f);
		}
		std::printf("varies %d\n", distinct > 0 ? 1 : 0);
		std::printf("alpha_kept %d\n", opaque == int(W * H) ? 1 : 0);
		return 0;
	});
}
