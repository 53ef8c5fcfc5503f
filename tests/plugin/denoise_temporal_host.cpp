// denoise_temporal_host.cpp — the denoiser's temporal stage through the plugin boundary: dlopen "HipRT.so", drive the
// rfw::RenderContext through its VIRTUAL interface (get_settings must list "DENOISE_TEMPORAL" with "0" / "1"; DENOISE and
// DENOISE_TEMPORAL on; a camera that moves every frame, Reset every frame), and compare every image render_frame hands out
// (RFWHIP_FRAMES_IN_FLIGHT of the environment: frame k - n + 1) bit for bit with the images of a context driven through the C ABI
// directly (rfwhip_read_framebuffer after each render, denoise and denoise_temporal on).  The history follows the presented
// frames: with n frames in flight the plugin presents frames 0 .. FRAMES - n, each once, in order, as the C ABI context does.
// The reference context renders BEFORE the plugin is opened.
#include "host_common.h"

static const int FRAMES = 6;

static rfw::Camera camera(int k)
{
	rfw::Camera cam = camera();
	cam.position.x = 0.02f * (float)k; // a slow pan
	return cam;
}

// the C ABI's denoised images of frames 0 .. FRAMES - 1 (and the spatial-only filter of the last one)
static int reference(const SceneData &s, std::vector<std::vector<float>> &den, std::vector<float> &raw)
{
	rfwhip_context *c = nullptr;
	ABI(rfwhip_create(0, 0, 1, &c));
	ABI(rfwhip_init(c, W, H));
	ABI(rfwhip_set_setting(c, "integrator", "pt"));
	ABI(rfwhip_set_setting(c, "denoise", "1"));
	ABI(rfwhip_set_setting(c, "denoise_temporal", "1"));
	if (int r = upload_abi(c, s))
		return r;
	den.assign(FRAMES, std::vector<float>(size_t(W) * H * 4));
	for (int k = 0; k < FRAMES; k++)
	{
		const rfwhip_camera cam = pod(camera(k));
		ABI(rfwhip_render(c, &cam, RFWHIP_RESET));
		ABI(rfwhip_wait(c));
		ABI(rfwhip_read_framebuffer(c, den[k].data()));
	}
	// the last frame's spatial-only filter: the temporal output must differ from it
	raw.assign(size_t(W) * H * 4, 0.0f);
	ABI(rfwhip_set_setting(c, "denoise", "0"));
	ABI(rfwhip_read_framebuffer(c, raw.data()));
	ABI(rfwhip_denoise_image(c, raw.data(), raw.data()));
	rfwhip_destroy(c);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const int in_flight = std::getenv("RFWHIP_FRAMES_IN_FLIGHT") ? std::max(1, std::atoi(std::getenv("RFWHIP_FRAMES_IN_FLIGHT"))) : 1;
	SceneData s(glm::vec3{0.25f, 0.5f, 0.75f});
	std::vector<std::vector<float>> want;
	std::vector<float> raw;
	if (int rc = reference(s, want, raw))
		return rc;
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadFramebuffer"}))
		return r;
	auto readfb = (ReadFn)p.sym[0];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		upload(ctx, s, [&] {
			const rfw::AvailableRenderSettings st = ctx->get_settings();
			int listed = 0;
			for (size_t i = 0; i < st.settingKeys.size(); i++)
				if (st.settingKeys[i] == "DENOISE_TEMPORAL" && i < st.settingValues.size() && st.settingValues[i] == std::vector<std::string>{"0", "1"})
					listed = 1;
			std::printf("listed %d\n", listed);
			ctx->set_setting(rfw::RenderSetting("DENOISE", "1"));
			ctx->set_setting(rfw::RenderSetting("DENOISE_TEMPORAL", "1"));
		});
		std::vector<float> img(size_t(W) * H * 4);
		int equal = 0;
		for (int k = 0; k < FRAMES; k++)
		{
			ctx->render_frame(camera(k), rfw::Reset);
			if (readfb(ctx, img.data()) != 0)
				rc = 4;
			// what render_frame hands out with n frames in flight: frame k - n + 1 (frame 0 until there is an older one)
			const int shown = std::max(0, k - in_flight + 1);
			equal += std::memcmp(img.data(), want[(size_t)shown].data(), img.size() * sizeof(float)) == 0;
		}
		std::printf("frames %d equal %d\n", FRAMES, equal);
		std::printf("differs_from_spatial %d\n", std::memcmp(want.back().data(), raw.data(), raw.size() * sizeof(float)) != 0 ? 1 : 0);
		return 0;
	});
}
