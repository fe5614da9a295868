// Stand-alone check of the host chain of the sharded numpy-order moments (np_shard_sum, csrc/moments_np.hip) on the CPU: the
// unit is included whole, the ranks' parts are formed with its own host routines, no HIP call is made and no GPU is needed.
// Sharded sums must equal the chain over the whole array bit for bit, and slots that do not tile the raster must be refused.
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Itopo_descriptors_amd/csrc -Iinclude tools/np_shard_sum_check.cpp -o /tmp/np_shard_sum_check && /tmp/np_shard_sum_check
#include "moments_np.hip"
#include <cstdarg>
#include <cstdio>
namespace topo {
static Context g_ctx;
Context& ctx() { return g_ctx; }
void set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vfprintf(stderr, fmt, a); va_end(a); fputc('\n', stderr); }
int workspace(int, size_t, void**) { return TOPO_AMD_EINVAL; }
}
using namespace topo;
static uint32_t bits(float f) { uint32_t w; std::memcpy(&w, &f, 4); return w; }
static float whole(const std::vector<float>& a, size_t chunk) {
    float s = 0.0f;
    for (size_t at = 0; at < a.size(); at += chunk) s = s + pairwise_host(a.data() + at, std::min(chunk, a.size() - at));
    return s;
}
static int run(size_t count, size_t chunk, const std::vector<size_t>& cuts, unsigned seed) {
    std::vector<float> a(count);
    uint32_t x = seed * 2654435761u + 1;
    for (auto& v : a) { x = x * 1664525u + 1013904223u; v = 1800.0f + (float)(x >> 8) * (1.0f / 16777216.0f) * 900.0f; }
    const int slots = (int)cuts.size();
    float sum = 0, sum2 = 0;
    std::vector<uint32_t> w1(np_shard_words(count, chunk, slots, true), 0), w2(np_shard_words(count, chunk, slots, false), 0);
    const size_t per = np_per(chunk), cap = np_frag_cap(count, chunk);
    auto fill = [&](std::vector<uint32_t>& w, bool sq, float mean) {
        size_t first = 0;
        for (int s = 0; s < slots; ++s) {
            const size_t n = cuts[s];
            const NpWindow win = np_window(first, n, chunk);
            for (size_t k = win.c0; k < win.c1; ++k)
                for (size_t i = 0; i < chunk / per; ++i) {
                    std::vector<float> t(a.begin() + k * chunk + i * per, a.begin() + k * chunk + (i + 1) * per);
                    if (sq) for (auto& v : t) { float d = v - mean; v = d * d; }
                    w[k * (chunk / per) + i] = bits(pairwise_host(t.data(), per));
                }
            if (!sq) {
                uint32_t* area = w.data() + np_shard_partials(count, chunk) + (size_t)(slots - 1 - s) * (kNpSlotHeader + 2 * cap);  // slots in reverse order
                area[0] = (uint32_t)first, area[1] = (uint32_t)((uint64_t)first >> 32), area[2] = (uint32_t)n, area[3] = (uint32_t)((uint64_t)n >> 32);
                for (size_t i = 0; i < win.head; ++i) area[4 + i] = bits(a[first + i]);
                for (size_t i = 0; i < win.tail; ++i) area[4 + cap + i] = bits(a[first + n - win.tail + i]);
            }
            first += n;
        }
    };
    fill(w1, false, 0);
    if (np_shard_sum(w1.data(), w1.data(), count, chunk, slots, false, 0, &sum) != 0) return 1;
    const float want = whole(a, chunk), mean = sum / (float)count;
    fill(w2, true, mean);
    if (np_shard_sum(w2.data(), w1.data(), count, chunk, slots, true, mean, &sum2) != 0) return 1;
    std::vector<float> d(a);
    for (auto& v : d) { float e = v - mean; v = e * e; }
    const float want2 = whole(d, chunk);
    const bool ok = bits(sum) == bits(want) && bits(sum2) == bits(want2);
    printf("count %zu chunk %zu slots %d: %s (%.9g %.9g)\n", count, chunk, slots, ok ? "ok" : "MISMATCH", sum, sum2);
    return ok ? 0 : 1;
}
int main() {
    int bad = 0;
    bad += run(56 * 203, 128, {5 * 203, 203, 203, 9 * 203, 40 * 203}, 1);
    bad += run(56 * 51, 128, {5 * 51, 51, 51, 9 * 51, 40 * 51}, 2);
    bad += run(16 * 256, 1024, {1024, 1024, 2048}, 3);
    bad += run(192 * 520, 8192, {64 * 520, 64 * 520, 64 * 520}, 4);
    bad += run(120 * 203, 8192, {8120, 8120, 8120}, 5);
    bad += run(100, 8192, {30, 70}, 6);
    bad += run(300 * 1003, 32768, {100 * 1003, 77 * 1003, 123 * 1003}, 7);
    bad += run(5, 128, {1, 1, 1, 1, 1}, 8);
    // slots that do not tile the raster are refused
    {
        std::vector<uint32_t> w(np_shard_words(1000, 128, 2, true), 0);
        uint32_t* a0 = w.data() + np_shard_partials(1000, 128);
        a0[2] = 400;
        uint32_t* a1 = a0 + 4 + 2 * 128;
        a1[0] = 500, a1[2] = 500;
        float s;
        bad += np_shard_sum(w.data(), w.data(), 1000, 128, 2, false, 0, &s) == TOPO_AMD_EINVAL ? 0 : 1;
    }
    printf(bad ? "FAILED\n" : "all ok\n");
    return bad;
}
