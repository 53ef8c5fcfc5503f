// noise_host.cpp — the noise estimate through the plugin boundary: dlopen "HipRT.so", drive the rfw::RenderContext through its
// virtual interface for a RESET frame and two CONVERGE frames, and compare what hiprtGetNoise answers with rfwhip_group_get_noise of
// a group driven through the C ABI directly on the same scene.  With RFWHIP_NOISE=1 in the environment the two records are equal
// byte for byte; without it hiprtGetNoise refuses with RFWHIP_ERR_STATE and nothing else changes.  The reference group renders
// BEFORE the plugin is opened.
#include "host_common.h"

typedef int (*NoiseFn)(rfw::RenderContext *, rfwhip_noise_stats *);

static const int FRAMES = 3;

// the C ABI's answer after FRAMES frames
static int reference(const SceneData &s, rfwhip_noise_stats *want)
{
	rfwhip_group *g = nullptr;
	if (int r = reference_group(&g))
		return r;
	ABI(rfwhip_group_set_setting(g, "noise_estimate", "1"));
	if (int r = upload_abi(g, s))
		return r;
	const rfwhip_camera cam = pod(camera());
	for (int k = 0; k < FRAMES; k++)
		ABI(rfwhip_group_render(g, &cam, k == 0 ? RFWHIP_RESET : RFWHIP_CONVERGE));
	ABI(rfwhip_group_get_noise(g, want));
	rfwhip_group_destroy(g);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const bool on = std::getenv("RFWHIP_NOISE") && std::string(std::getenv("RFWHIP_NOISE")) == "1";
	SceneData s(glm::vec3{0.25f, 0.5f, 0.75f});
	rfwhip_noise_stats want;
	std::memset(&want, 0, sizeof(want));
	if (int rc = reference(s, &want))
		return rc;
	Plugin p;
	if (int r = p.open(dir, {"hiprtGetNoise"}))
		return r;
	auto get_noise = (NoiseFn)p.sym[0];
	return drive(p, [&](rfw::RenderContext *ctx, int &) {
		upload(ctx, s);
		const rfw::Camera cam = camera();
		rfwhip_noise_stats got;
		std::memset(&got, 0, sizeof(got));
		int first = -1, last = -1;
		for (int k = 0; k < FRAMES; k++)
		{
			ctx->render_frame(cam, k == 0 ? rfw::Reset : rfw::Converge);
			last = get_noise(ctx, &got);
			if (k == 0)
				first = last;
		}
		// one sample: no estimate yet; then the C ABI's record (on), or a refusal every time (off)
		std::printf("on %d\n", on ? 1 : 0);
		std::printf("first %d\n", first);
		std::printf("last %d\n", last);
		std::printf("equal %d\n", std::memcmp(&got, &want, sizeof(got)) == 0 ? 1 : 0);
		std::printf("stats %llu %llu %llu %.9g %.9g\n", (unsigned long long)got.samples, (unsigned long long)got.pixels,
					(unsigned long long)got.converged, got.mean_error, (double)got.max_error);
		return 0;
	});
}
