// TEST INFRASTRUCTURE — not part of the product.
//
// A stand-alone host for libgama_vtm_plugin.so that loads it the way GamaTTS's plugin loader does
// (model = 2000: dlopen(dll_path, RTLD_NOW), the two symbols of include/gama_vtm_plugin.h, the returned
// pointer used as a VocalTractModel*, the destruct symbol called before dlclose) and drives it with the same
// two caller contracts as oracle/ref_driver.cpp: Controller::synthesize's per-sample loop (batch protocol) and
// the editor's polled outputBuffer() (interactive protocol).  It needs none of the reference's sources, so the
// plugin tests run in any checkout; where oracle/_ref/ref_vtm exists the tests drive the plugin through that
// binary as well and require the same samples from both.
//
// usage (the arguments of oracle/ref_driver.cpp's plugin mode):
//   vtm_plugin_host <config.txt> 2000:<plugin.so> <output_rate> <control_rate> <params.f32>
//                   <n_frames> <out.f32|-> [repeat] [poll=<nframes>]
// prints one line:  N=<samples> steps=<internal steps> fs=<internal rate> sec=<wall> ns_per_step=<...>
//                   [callbacks=<n>]
#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../include/gama_vtm_plugin.h"

// Both types below need external linkage: in an anonymous namespace the compiler sees that no class in this file
// derives from VocalTractModel and turns the calls through the plugin's object into calls of its pure virtuals.
namespace gvtm_plugin_host {

// The host's configuration object as the plugin reads it (include/gama_vtm_plugin.h: two strings, then the
// key/value map).
struct ConfigurationData {
	std::string filePath;
	std::string dirPath;
	std::unordered_map<std::string, std::string> valueMap;
};

// The VocalTractModel interface in the order include/gama_vtm_plugin.h documents.
class VocalTractModel {
public:
	virtual ~VocalTractModel() noexcept = default;
	virtual void reset() noexcept = 0;
	virtual double internalSampleRate() const noexcept = 0;
	virtual double outputSampleRate() const noexcept = 0;
	virtual void setParameter(int parameter, float value) noexcept = 0;
	virtual void setAllParameters(const std::vector<float>& parameters) noexcept = 0;
	virtual void execSynthesisStep() noexcept = 0;
	virtual void finishSynthesis() noexcept = 0;
	virtual std::vector<float>& outputBuffer() noexcept = 0;
};

} // namespace gvtm_plugin_host

using gvtm_plugin_host::ConfigurationData;
using gvtm_plugin_host::VocalTractModel;

namespace {

std::string trim(const std::string& s)
{
	const auto b = s.find_first_not_of(" \t\r");
	if (b == std::string::npos) return std::string();
	const auto e = s.find_last_not_of(" \t\r");
	return s.substr(b, e - b + 1);
}

// `key = value` lines, `#` comments (the voice file format, gama_tts_amd.read_config_file).
bool readConfig(const char* path, ConfigurationData& cfg)
{
	std::ifstream in(path);
	if (!in) return false;
	cfg.filePath = path;
	const std::string p(path);
	const auto slash = p.rfind('/');
	cfg.dirPath = slash == std::string::npos ? std::string() : p.substr(0, slash + 1);
	std::string line;
	while (std::getline(in, line)) {
		if (line.empty() || line[0] == '#') continue;
		const auto eq = line.find('=');
		if (eq == std::string::npos) continue;
		cfg.valueMap[trim(line.substr(0, eq))] = trim(line.substr(eq + 1));
	}
	return true;
}

// Copies up to n samples from buf[pos..] and empties buf once all of it has been read (the editor's drain).
std::size_t drain(std::vector<float>& buf, std::size_t& pos, float* out, std::size_t n)
{
	std::size_t k = 0;
	while (k < n && pos < buf.size()) out[k++] = buf[pos++];
	if (!buf.empty() && pos == buf.size()) {
		buf.clear();
		pos = 0;
	}
	return k;
}

// The per-step parameter vectors of the driver loop: each frame held for controlSteps steps, linearly
// interpolated towards the next one in float, the last frame repeated as the target of the last ramp.
std::vector<std::vector<float>> stepParameters(const std::vector<std::vector<float>>& frames, unsigned int controlSteps)
{
	std::vector<std::vector<float>> steps;
	if (frames.empty()) return steps;
	std::vector<std::vector<float>> list = frames;
	list.push_back(list.back());
	const std::size_t numParam = frames[0].size();
	const float coef = 1.0f / controlSteps;
	std::vector<float> cur(numParam), delta(numParam);
	for (std::size_t i = 1; i < list.size(); ++i) {
		for (std::size_t j = 0; j < numParam; ++j) {
			cur[j] = list[i - 1][j];
			delta[j] = (list[i][j] - cur[j]) * coef;
		}
		for (unsigned int s = 0; s < controlSteps; ++s) {
			steps.push_back(cur);
			for (std::size_t k = 0; k < numParam; ++k) cur[k] += delta[k];
		}
	}
	return steps;
}

bool writeSamples(const char* path, const std::vector<float>& x)
{
	if (std::strcmp(path, "-") == 0) return true;
	FILE* f = std::fopen(path, "wb");
	if (!f) {
		std::perror(path);
		return false;
	}
	std::fwrite(x.data(), sizeof(float), x.size(), f);
	std::fclose(f);
	return true;
}

} // namespace

int main(int argc, char** argv)
{
	if (argc < 8 || std::strncmp(argv[2], "2000:", 5) != 0) {
		std::fprintf(stderr, "usage: %s config 2000:plugin.so output_rate control_rate params.f32 n_frames out.f32|- [repeat] [poll=N]\n", argv[0]);
		return 2;
	}
	ConfigurationData cfg;
	if (!readConfig(argv[1], cfg)) {
		std::perror(argv[1]);
		return 2;
	}
	const char* dllPath = argv[2] + 5;
	cfg.valueMap["model"] = "2000";
	cfg.valueMap["dll_path"] = dllPath;
	cfg.valueMap["output_rate"] = argv[3];
	const double controlRate = std::atof(argv[4]);
	const std::size_t nFrames = std::strtoul(argv[6], nullptr, 10);
	const int repeat = argc > 8 ? std::atoi(argv[8]) : 1;
	const std::size_t pollFrames = (argc > 9 && std::strncmp(argv[9], "poll=", 5) == 0) ? std::strtoul(argv[9] + 5, nullptr, 10) : 0;
	const std::size_t numParam = 16;

	std::vector<std::vector<float>> frames(nFrames, std::vector<float>(numParam));
	{
		FILE* f = std::fopen(argv[5], "rb");
		if (!f) {
			std::perror(argv[5]);
			return 2;
		}
		for (auto& fr : frames) {
			if (std::fread(fr.data(), sizeof(float), numParam, f) != numParam) {
				std::fprintf(stderr, "short read on %s\n", argv[5]);
				std::fclose(f);
				return 2;
			}
		}
		std::fclose(f);
	}

	void* dll = dlopen(dllPath, RTLD_NOW);
	if (!dll) {
		std::fprintf(stderr, "dlopen: %s\n", dlerror());
		return 1;
	}
	using Construct = void* (*)(const void*, int);
	using Destruct = void (*)(void*);
	auto construct = reinterpret_cast<Construct>(dlsym(dll, "GAMA_TTS_construct_vocal_tract_model"));
	auto destruct = reinterpret_cast<Destruct>(dlsym(dll, "GAMA_TTS_destruct_vocal_tract_model"));
	if (!construct || !destruct) {
		std::fprintf(stderr, "dlsym: %s\n", dlerror());
		return 1;
	}
	auto* vtm = static_cast<VocalTractModel*>(construct(&cfg, pollFrames > 0 ? 1 : 0));
	if (!vtm) {
		std::fprintf(stderr, "could not construct the vocal tract model\n");
		return 1;
	}
	const unsigned int controlSteps = static_cast<unsigned int>(std::rint(vtm->internalSampleRate() / controlRate));
	const std::vector<std::vector<float>> stepParams = stepParameters(frames, controlSteps);

	int rc = 0;
	const auto t0 = std::chrono::steady_clock::now();
	if (pollFrames > 0) {
		// one callback asks for pollFrames samples: drain what is there, then step until enough is there
		std::vector<float> drained, callback(pollFrames);
		std::vector<float>& buffer = vtm->outputBuffer();
		std::size_t bufferPos = 0, next = 0, callbacks = 0;
		bool finished = false;
		for (;;) {
			++callbacks;
			const std::size_t n = drain(buffer, bufferPos, callback.data(), pollFrames);
			drained.insert(drained.end(), callback.begin(), callback.begin() + n);
			if (n == pollFrames) continue;
			if (finished) break;
			const std::size_t target = pollFrames - n;
			while (buffer.size() < target && next < stepParams.size()) {
				for (std::size_t i = 0; i < numParam; ++i) vtm->setParameter(static_cast<int>(i), stepParams[next][i]);
				vtm->execSynthesisStep();
				++next;
			}
			if (buffer.size() < target) {
				vtm->finishSynthesis();
				finished = true;
			}
			const std::size_t n2 = drain(buffer, bufferPos, callback.data(), target);
			drained.insert(drained.end(), callback.begin(), callback.begin() + n2);
		}
		const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (!writeSamples(argv[7], drained)) rc = 2;
		std::printf("N=%zu steps=%zu fs=%.17g sec=%.6f ns_per_step=%.2f callbacks=%zu\n", drained.size(), stepParams.size(),
				vtm->internalSampleRate(), sec, stepParams.empty() ? 0.0 : sec * 1e9 / stepParams.size(), callbacks);
	} else {
		std::size_t steps = 0;
		for (int r = 0; r < repeat; ++r) {
			if (!vtm->outputBuffer().empty()) vtm->reset();
			for (const auto& p : stepParams) {
				vtm->setAllParameters(p);
				vtm->execSynthesisStep();
			}
			steps += stepParams.size();
			vtm->finishSynthesis();
		}
		const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		const std::vector<float>& out = vtm->outputBuffer();
		if (!writeSamples(argv[7], out)) rc = 2;
		std::printf("N=%zu steps=%zu fs=%.17g sec=%.6f ns_per_step=%.2f\n", out.size(), steps, vtm->internalSampleRate(), sec,
				steps ? sec * 1e9 / steps : 0.0);
	}
	destruct(vtm);
	dlclose(dll);
	return rc;
}
