// denoise_host.cpp — the denoiser through the plugin boundary: dlopen "HipRT.so", drive the rfw::RenderContext through its VIRTUAL
// interface (get_settings must list the reference's "DENOISE" key with "0" / "1", set_setting("DENOISE", "1"), render_frame), and
// compare every image render_frame hands out (RFWHIP_FRAMES_IN_FLIGHT of the environment: frame k - n + 1) bit for bit with the
// denoised image of a context driven through the C ABI directly (rfwhip_read_framebuffer with denoise=1) on the same scene.  The
// reference context renders BEFORE the plugin is opened.
#include "host_common.h"

static const int FRAMES = 6;

// the C ABI's denoised images of frames 0 .. FRAMES - 1 (and the raw image of the last one)
static int reference(const SceneData &s, std::vector<std::vector<float>> &den, std::vector<float> &raw)
{
	rfwhip_context *c = nullptr;
	ABI(rfwhip_create(0, 0, 1, &c));
	ABI(rfwhip_init(c, W, H));
	ABI(rfwhip_set_setting(c, "integrator", "pt"));
	ABI(rfwhip_set_setting(c, "denoise", "1"));
	if (int r = upload_abi(c, s))
		return r;
	const rfwhip_camera cam = pod(camera());
	den.assign(FRAMES, std::vector<float>(size_t(W) * H * 4));
	for (int k = 0; k < FRAMES; k++)
	{
		ABI(rfwhip_render(c, &cam, k == 0 ? RFWHIP_RESET : RFWHIP_CONVERGE));
		ABI(rfwhip_wait(c));
		ABI(rfwhip_read_framebuffer(c, den[k].data()));
	}
	raw.assign(size_t(W) * H * 4, 0.0f);
	ABI(rfwhip_set_setting(c, "denoise", "0"));
	ABI(rfwhip_read_framebuffer(c, raw.data()));
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
				if (st.settingKeys[i] == "DENOISE" && i < st.settingValues.size() && st.settingValues[i] == std::vector<std::string>{"0", "1"})
					listed = 1;
			std::printf("listed %d\n", listed);
			ctx->set_setting(rfw::RenderSetting("DENOISE", "1"));
		});
		const rfw::Camera cam = camera();
		std::vector<float> img(size_t(W) * H * 4);
		int equal = 0;
		for (int k = 0; k < FRAMES; k++)
		{
			ctx->render_frame(cam, k == 0 ? rfw::Reset : rfw::Converge);
			if (readfb(ctx, img.data()) != 0)
				rc = 4;
			// what render_frame hands out with n frames in flight: frame k - n + 1 (frame 0 until there is an older one)
			const int shown = std::max(0, k - in_flight + 1);
			equal += std::memcmp(img.data(), want[(size_t)shown].data(), img.size() * sizeof(float)) == 0;
		}
		std::printf("frames %d equal %d\n", FRAMES, equal);
		std::printf("differs_from_raw %d\n", std::memcmp(want.back().data(), raw.data(), raw.size() * sizeof(float)) != 0 ? 1 : 0);
		return 0;
	});
}
