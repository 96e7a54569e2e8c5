// tests/test_environment_host.py: jpt_host.hpp load_hdr on a file -> "<width> <height>\n" and the floats, raw, on stdout;
// exit status 2 and the message on stderr when the file is refused.
#include <jpt_host.hpp>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char** argv)
{
    if (argc != 2) return 1;
    std::ifstream f(argv[1], std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    std::vector<float> rgb;
    int32_t w = 0, h = 0;
    try {
        jpt_host::load_hdr(ss.str(), rgb, w, h);
    } catch (const std::exception& e) {
        std::cerr << e.what() << "\n";
        return 2;
    }
    std::printf("%d %d\n", (int)w, (int)h);
    std::fwrite(rgb.data(), sizeof(float), rgb.size(), stdout);
    return 0;
}
