// PyTorch bindings of the wire audio ingest library (_vwa_ingest.so).  Rules and check vocabulary:
// csrc/torch_checks.h.
#include "torch_checks.h"
#include "ingest/ingest.h"

namespace {

using namespace vwa::checks;

// (L, M, H) of a supported rate
std::tuple<int64_t, int64_t, int64_t> geometry(int64_t sample_rate) {
  int L = 0, M = 0, H = 0;
  TORCH_CHECK(sample_rate > 0 && sample_rate <= 48000 && vwa_ingest_geometry((int)sample_rate, &L, &M, &H) == 0,
              "sample_rate must be one of 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, not ",
              sample_rate);
  return {L, M, H};
}

// raw is the anchor; its byte count is the call's window
void ingest(const Tensor& raw, int64_t encoding, int64_t sample_rate, int64_t channels, int64_t channel,
            const Tensor& table, const Tensor& out) {
  // the format and the shapes first (host metadata: a host tensor gets this far), the devices after
  TORCH_CHECK(encoding == kIngestLinear16 || encoding == kIngestMulaw || encoding == kIngestAlaw,
              "encoding must be 0 (linear16), 1 (mulaw) or 2 (alaw), not ", encoding);
  const auto [L, M, H] = geometry(sample_rate);
  TORCH_CHECK(channels >= 1 && channels <= kIngestMaxChannels, "channels must be in [1, ", kIngestMaxChannels,
              "], not ", channels);
  TORCH_CHECK(channel >= -1 && channel < channels, "channel must be -1 (downmix) or in [0, ", channels, "), not ",
              channel);
  TORCH_CHECK(raw.scalar_type() == at::kByte && raw.dim() == 1 && raw.is_contiguous(),
              "raw must be contiguous 1-D ", at::kByte, ", not ", raw.scalar_type(), " ", raw.sizes());
  const int64_t frame = channels * (encoding == kIngestLinear16 ? 2 : 1);
  TORCH_CHECK(raw.numel() % frame == 0, "raw must hold whole frames of ", frame, " bytes, not ", raw.numel(),
              " bytes");
  const int64_t n_in = raw.numel() / frame;
  TORCH_CHECK(n_in <= kIngestMaxFrames, "raw must hold <= ", kIngestMaxFrames, " frames, not ", n_in);
  TORCH_CHECK(table.scalar_type() == at::kFloat && table.dim() == 2 && table.is_contiguous() && table.size(0) == L &&
                  table.size(1) == 2 * H,
              "table must be contiguous ", at::kFloat, " [", L, ", ", 2 * H, "] for sample_rate ", sample_rate,
              ", not ", table.scalar_type(), " ", table.sizes());
  const int64_t n_out = n_in * L / M;
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.dim() == 1 && out.is_contiguous() && out.numel() >= n_out,
              "out must be contiguous 1-D ", at::kFloat, " with >= ", n_out, " elements, not ", out.scalar_type(), " ",
              out.sizes());
  check_vec_1d(raw, raw, at::kByte, 0, "raw");
  check_gpu(table, raw, at::kFloat, "table");
  check_vec_1d(out, raw, at::kFloat, n_out, "out");
  TORCH_CHECK(encoding != kIngestLinear16 || aligned(raw, 2), "raw must be 2-byte aligned for linear16");
  TORCH_CHECK(!overlaps(out.data_ptr(), 4 * n_out, raw.data_ptr(), raw.numel()), "out must not overlap raw");
  TORCH_CHECK(!overlaps(out.data_ptr(), 4 * n_out, table.data_ptr(), 4 * table.numel()),
              "out must not overlap table");

  const c10::DeviceGuard guard(raw.device());
  check_rc(vwa_ingest(raw.data_ptr<uint8_t>(), n_in, (int)encoding, (int)channels, (int)channel, (int)sample_rate,
                      table.data_ptr<float>(), out.data_ptr<float>(), out.numel(), cur_stream(raw)),
           "ingest");
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "gfx950 wire audio ingest: s16le / G.711, 1..8 channels, 8..48 kHz -> 16 kHz f32 mono";
  m.attr("MAX_CHANNELS") = kIngestMaxChannels;
  m.attr("MAX_FRAMES") = kIngestMaxFrames;
  m.def("geometry", &geometry, py::arg("sample_rate"));
  m.def("ingest", &ingest, py::arg("raw"), py::arg("encoding"), py::arg("sample_rate"), py::arg("channels"),
        py::arg("channel"), py::arg("table"), py::arg("out"));
}
