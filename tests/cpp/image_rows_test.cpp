// image_rows_test.cpp -- the partition's arithmetic (csrc/jpt_image.cpp: jpt::rows_of_rank, jpt::max_rows_of_any_rank, jpt::scatter_rows)
// on the host: no context, no device.  For every height, world and width below it checks that the ranks' row counts sum to the height,
// that scattering every rank's padded piece into one zeroed image writes each image row exactly once and from the right local row, and
// that the largest share is what the piece size reports; and prints the image rows of every rank in the order of its buffers, which
// tests/test_image_rows_host.py (it builds and runs this program) compares with gdpathtracing_amd/partition.py.
#include "../../gdpathtracing_amd/csrc/jpt_ctx.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int g_failed = 0;
void check(bool ok, const char* what, int32_t h, int32_t world, int32_t w)
{
    if (ok) return;
    std::fprintf(stderr, "height %d world %d width %d: %s\n", h, world, w, what);
    g_failed++;
}

// the pixel of local row `ly` of `rank`, column `x`: never 0, and different for every (rank, ly, x) of a case
uint32_t pixel(int32_t rank, int32_t ly, int32_t x) { return ((uint32_t)(rank + 1) << 24) | ((uint32_t)(ly + 1) << 8) | (uint32_t)(x + 1); }

void one_case(int32_t h, int32_t world, int32_t w)
{
    const int32_t piece_rows = max_rows_of_any_rank(h, world);
    int32_t sum = 0, largest = 0;
    for (int32_t r = 0; r < world; r++) {
        const int32_t n = rows_of_rank(h, r, world);
        check(n >= 0 && n <= piece_rows, "a rank's share is larger than the piece", h, world, w);
        sum += n;
        if (n > largest) largest = n;
    }
    check(sum == h, "the ranks' rows do not sum to the height", h, world, w);
    check(largest == piece_rows, "the piece is not the largest share", h, world, w);

    std::vector<uint32_t> image((size_t)h * w, 0u);
    std::vector<int> written((size_t)h, 0);
    for (int32_t r = 0; r < world; r++) {
        const int32_t n = rows_of_rank(h, r, world);
        // the rank's piece, padded to the piece size as its buffers are; the padding is 0 and must not arrive anywhere
        std::vector<uint32_t> piece((size_t)piece_rows * w, 0u);
        for (int32_t ly = 0; ly < n; ly++)
            for (int32_t x = 0; x < w; x++) piece[(size_t)ly * w + x] = pixel(r, ly, x);
        std::vector<uint32_t> alone((size_t)h * w, 0u);
        scatter_rows(reinterpret_cast<const char*>(piece.data()), reinterpret_cast<char*>(alone.data()), w, h, r, world, sizeof(uint32_t));
        scatter_rows(reinterpret_cast<const char*>(piece.data()), reinterpret_cast<char*>(image.data()), w, h, r, world, sizeof(uint32_t));
        // which image row each local row went to, in the order of the buffer
        std::printf("rows %d %d %d %d:", h, world, w, r);
        int32_t next = 0;
        std::vector<int32_t> at((size_t)n, -1);
        for (int32_t y = 0; y < h; y++) {
            const uint32_t first = alone[(size_t)y * w];
            if (first == 0u) {
                for (int32_t x = 0; x < w; x++) check(alone[(size_t)y * w + x] == 0u, "a row is written in part", h, world, w);
                continue;
            }
            written[(size_t)y]++;
            const int32_t ly = (int32_t)((first >> 8) & 0xffffu) - 1;
            check((first >> 24) == (uint32_t)(r + 1) && ly >= 0 && ly < n, "a row holds another rank's or the padding's pixels", h, world, w);
            for (int32_t x = 0; x < w; x++) check(alone[(size_t)y * w + x] == pixel(r, ly, x), "a row is not its local row", h, world, w);
            if (ly >= 0 && ly < n) at[(size_t)ly] = y;
            next++;
        }
        check(next == n, "a rank wrote another number of rows than its share", h, world, w);
        for (int32_t ly = 0; ly < n; ly++) {
            check(at[(size_t)ly] >= 0, "a local row went nowhere", h, world, w);
            std::printf(" %d", at[(size_t)ly]);
        }
        std::printf("\n");
    }
    for (int32_t y = 0; y < h; y++) {
        check(written[(size_t)y] == 1, "an image row is not written exactly once", h, world, w);
        for (int32_t x = 0; x < w; x++) check(image[(size_t)y * w + x] != 0u, "the image has a hole", h, world, w);
    }
    std::printf("piece %d %d %d: %d\n", h, world, w, piece_rows);
}

}  // namespace

int main()
{
    const int32_t heights[] = {0, 1, 7, 8, 9, 20, 24, 65}, worlds[] = {1, 2, 3, 5}, widths[] = {1, 3};
    for (int32_t h : heights)
        for (int32_t world : worlds)
            for (int32_t w : widths) one_case(h, world, w);
    if (g_failed) std::fprintf(stderr, "%d checks failed\n", g_failed);
    return g_failed ? 1 : 0;
}
