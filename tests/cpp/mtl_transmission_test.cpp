// mtl_transmission_test.cpp -- include/jpt_host.hpp's load_mtl with and without its transmission parameter, for
// tests/test_transmission_host.py: prints one line per material, "name transmission ior albedo_r roughness", in name order.
// usage: mtl_transmission_test FILE.mtl 0|1
#include <cstdio>
#include <fstream>
#include <sstream>

#include "jpt_host.hpp"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::ifstream f(argv[1]);
    std::stringstream ss;
    ss << f.rdbuf();
    std::vector<std::string> maps;
    const auto mats = argv[2][0] == '1' ? jpt_host::load_mtl(ss.str(), maps, true) : jpt_host::load_mtl(ss.str(), maps);
    for (const auto& kv : mats)
        std::printf("%s %.9g %.9g %.9g %.9g\n", kv.first.c_str(), kv.second.transmission, kv.second.ior, kv.second.albedo.r, kv.second.roughness);
    return 0;
}
