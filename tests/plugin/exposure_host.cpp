// exposure_host.cpp — the exposure meter through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY and RFWHIP_EXPOSURE
// (and RFWHIP_EXPOSURE_SPEED) set in the environment, drive the rfw::RenderContext through its virtual interface, and compare the
// bytes hiprtReadDisplay returns after every render_frame (RFWHIP_FRAMES_IN_FLIGHT of the environment: frame k - n + 1) with the
// bytes rfwhip_group_read_display gives for the same frames of a group driven through the C ABI directly, on the same scene with
// the same display_tonemap and display_exposure* settings; then hiprtGetExposure's record against that group's.  The plugin is
// created FIRST: a value of RFWHIP_EXPOSURE it refuses ends the program (exit status 5, the message on stderr) before anything renders.
#include "host_common.h"

typedef int (*ExposureFn)(rfw::RenderContext *, rfwhip_meter_stats *);

static const int FRAMES = 5;

// the C ABI's display images (RGBA8) of frames 0 .. FRAMES - 1, and the meter's record behind the last one
static int reference(const SceneData &s, const char *tonemap, const char *exposure, const char *speed, std::vector<std::vector<uint8_t>> &want,
					 rfwhip_meter_stats &meter)
{
	rfwhip_group *g = nullptr;
	if (int r = reference_group(&g))
		return r;
	ABI(rfwhip_group_set_setting(g, "display_tonemap", tonemap));
	ABI(rfwhip_group_set_setting(g, "display_exposure", exposure));
	if (speed)
		ABI(rfwhip_group_set_setting(g, "display_exposure_speed", speed));
	if (int r = upload_abi(g, s))
		return r;
	const rfwhip_camera cam = pod(camera());
	want.assign(FRAMES, std::vector<uint8_t>(size_t(W) * H * 4));
	for (int k = 0; k < FRAMES; k++)
	{
		ABI(rfwhip_group_render(g, &cam, k == 0 ? RFWHIP_RESET : RFWHIP_CONVERGE));
		ABI(rfwhip_group_read_display(g, RFWHIP_DISPLAY_RGBA8, want[(size_t)k].data()));
	}
	ABI(rfwhip_group_get_meter(g, &meter));
	rfwhip_group_destroy(g);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const int in_flight = std::getenv("RFWHIP_FRAMES_IN_FLIGHT") ? std::max(1, std::atoi(std::getenv("RFWHIP_FRAMES_IN_FLIGHT"))) : 1;
	const char *tonemap = std::getenv("RFWHIP_DISPLAY") ? std::getenv("RFWHIP_DISPLAY") : "aces";
	const char *exposure = std::getenv("RFWHIP_EXPOSURE") ? std::getenv("RFWHIP_EXPOSURE") : "manual";
	const char *speed = std::getenv("RFWHIP_EXPOSURE_SPEED");
	SceneData s(glm::vec3{0.25f, 0.5f, 0.75f});
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadDisplay", "hiprtGetExposure"}))
		return r;
	auto read_display = (ReadDisplayFn)p.sym[0];
	auto get_exposure = (ExposureFn)p.sym[1];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		std::vector<std::vector<uint8_t>> want;
		rfwhip_meter_stats ref;
		if (int r = reference(s, tonemap, exposure, speed, want, ref))
			return r;
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
		rfwhip_meter_stats got;
		if (get_exposure(ctx, &got) != 0)
			rc = 4;
		std::printf("steps %u\n", got.steps);
		std::printf("record_equal %d\n", std::memcmp(&got, &ref, sizeof(got)) == 0 ? 1 : 0);
		std::printf("exposure %.9g\n", got.exposure);
		// the exposure does something: the first and the last frame differ (the accumulation converges AND the exposure adapts)
		std::printf("varies %d\n", want.front() != want.back() ? 1 : 0);
		return 0;
	});
}
