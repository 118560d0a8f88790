// dict_reader_check.cpp -- the meshQualityDict reader (smoothmesh_amd/csrc/host/quality_dict.cpp) on the fixtures of
// tests/golden/mesh_quality_dicts and on malformed inputs it writes itself; built with -fsanitize=address,undefined by
// tests/test_mesh_quality_dict.py.  usage: dict_reader_check <fixture dir> <scratch dir>; prints "ok <n> checks".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "quality_dict.hpp"

using namespace smhost;
namespace fs = std::filesystem;

static int g_checks = 0;

static void require(bool ok, const std::string& what) {
    ++g_checks;
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what.c_str());
        std::exit(1);
    }
}

static int keyIndex(const std::string& name) {
    for (int k = 0; k < kQualityDictKeys; ++k)
        if (name == kQualityDictKeyNames[k]) return k;
    require(false, "no such key " + name);
    return -1;
}

static MeshQualityDict readOk(const std::string& path, const std::vector<std::string>& etc = {}) {
    MeshQualityDict d;
    try { readMeshQualityDict(path, etc, d); }
    catch (const std::exception& e) { require(false, path + " should read: " + e.what()); }
    return d;
}

// the reader must throw, and the message must hold every piece of `pieces`
static void readFails(const std::string& path, const std::vector<std::string>& pieces, const std::vector<std::string>& etc = {}) {
    MeshQualityDict d;
    std::string msg;
    try { readMeshQualityDict(path, etc, d); }
    catch (const std::runtime_error& e) { msg = e.what(); }
    require(!msg.empty(), path + " should be refused");
    for (const std::string& p : pieces) require(msg.find(p) != std::string::npos, path + ": '" + msg + "' lacks '" + p + "'");
}

static void write(const fs::path& p, const std::string& text) {
    std::ofstream f(p, std::ios::binary);
    f << text;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string fix = fs::absolute(argv[1]).string();
    const fs::path tmp = argv[2];
    fs::create_directories(tmp);

    MeshQualityDict d = readOk(fix + "/full");
    const double full[kQualityDictKeys] = {62, 18, 3.5, 75, 0.55, 1e-13, 1e-15, 1e-12, 0.02, 0.001, 0.05, 0.01, 0.03};
    for (int k = 0; k < kQualityDictKeys; ++k) require(d.found[k] && d.value[k] == full[k], std::string("full: ") + kQualityDictKeyNames[k]);
    require(d.ignored == std::vector<std::string>({"nSmoothScale", "errorReduction", "relaxed", "minVolCollapseRatio"}), "full: ignored keys");

    d = readOk(fix + "/partial");
    int nFound = 0;
    for (int k = 0; k < kQualityDictKeys; ++k) nFound += d.found[k] ? 1 : 0;
    require(nFound == 3 && d.value[keyIndex("maxNonOrtho")] == 55 && d.value[keyIndex("minFlatness")] == 0.6 && d.value[keyIndex("minArea")] == 2e-9 && d.ignored.empty(),
            "partial");

    d = readOk(fix + "/sentinels");
    for (int k = 0; k < kQualityDictKeys; ++k) require(d.found[k], "sentinels: found");
    require(d.value[keyIndex("maxNonOrtho")] == 180 && d.value[keyIndex("minVol")] == -1e30 && d.value[keyIndex("minTwist")] == -1, "sentinels: values");

    d = readOk(fix + "/with_include");
    require(d.value[keyIndex("maxNonOrtho")] == 50 && d.value[keyIndex("minTwist")] == 0.04 && d.value[keyIndex("minFlatness")] == 0.6, "with_include: override order");

    d = readOk(fix + "/with_etc", {fix + "/nowhere", fix + "/etc"});
    require(d.value[keyIndex("maxNonOrtho")] == 64 && d.value[keyIndex("minFaceWeight")] == 0.02 && d.value[keyIndex("minVol")] == 1e-14, "with_etc: values");
    require(d.ignored == std::vector<std::string>({"relaxed"}), "with_etc: ignored");
    readFails(fix + "/with_etc", {"with_etc:2", "caseDicts/meshQualityDict", "none was given"});
    readFails(fix + "/with_etc", {"with_etc:2", "caseDicts/meshQualityDict", fix + "/nowhere"}, {fix + "/nowhere"});
    readFails(fix + "/err_etc_missing", {"err_etc_missing:1", "caseDicts/noSuchDict", fix + "/etc"}, {fix + "/etc"});

    d = readOk(fix + "/override");
    require(d.value[keyIndex("maxConcave")] == 60 && d.value[keyIndex("minVol")] == 1e-10 && d.ignored == std::vector<std::string>({"someList", "note"}), "override");

    readFails(fix + "/err_cycle_a", {"err_cycle_b:3", "include cycle"});
    readFails(fix + "/err_missing_include", {"err_missing_include:2", "no_such_file"});
    readFails(fix + "/err_macro", {"err_macro:2", "$limit"});
    readFails(fix + "/err_brace", {"err_brace:3", "unterminated {"});
    readFails(fix + "/err_comment", {"err_comment:2", "unterminated /*"});
    readFails(fix + "/err_semicolon", {"err_semicolon:1", "missing ;"});
    readFails(fix + "/err_nonnumeric", {"err_nonnumeric:2", "minFlatness", "half"});
    readFails(fix + "/err_nan", {"err_nan:3", "minArea", "NaN"});
    readFails(fix + "/err_directive", {"err_directive:1", "#inputMode"});
    readFails(fix + "/no_such_dict", {"no_such_dict", "cannot read"});

    // malformed inputs written here: ends of file in every place, odd bytes
    const std::vector<std::pair<std::string, std::string>> bad = {
        {"maxNonOrtho", "missing ;"}, {"maxNonOrtho 60", "missing ;"}, {"maxNonOrtho 60 70;", "one number"}, {"maxNonOrtho;", "one number"},
        {"maxNonOrtho \"60\";", "one number"}, {"maxNonOrtho 60x;", "not a number"}, {"maxNonOrtho 1e;", "not a number"}, {"}", "} without {"},
        {"{ a 1; }", "{ without a name"}, {"a { b { c 1; } ", "unterminated {"}, {"a \"open", "unterminated string"}, {"#include", "quoted file name"},
        {"#include partial", "quoted file name"}, {"#include \"$FOAM/x\"", "macro"}, {"$x 1;", "macro"}, {"/*", "unterminated /*"}, {"/", "missing ;"},
        {"a /* x */ { } } ", "} without {"}, {"maxNonOrtho -nan;", "NaN"}, {"\"name\" 1;", "a string where a keyword"}, {"a 1; #calc \"1\";", "#calc"},
        {"a #include;", "directive"}};
    int n = 0;
    for (const auto& b : bad) {
        const fs::path p = tmp / ("bad" + std::to_string(n++));
        write(p, b.first);
        readFails(p.string(), {p.filename().string() + ":1", b.second});
    }
    // well-formed odd inputs
    write(tmp / "odd", std::string("// only a comment"));
    d = readOk((tmp / "odd").string());
    require(d.ignored.empty(), "odd: comment only");
    write(tmp / "odd2", std::string("a\t1;;\r\nmaxNonOrtho\n{\n}\nminVol 1e-3/*c*/;//x\nminArea 0x10;\nminTwist inf;"));
    d = readOk((tmp / "odd2").string());
    require(!d.found[keyIndex("maxNonOrtho")] && d.value[keyIndex("minVol")] == 1e-3 && d.value[keyIndex("minArea")] == 16 && std::isinf(d.value[keyIndex("minTwist")]),
            "odd2: values");
    require(d.ignored == std::vector<std::string>({"a", "maxNonOrtho"}), "odd2: a sub-dictionary under a read key's name is ignored");
    write(tmp / "empty", "");
    d = readOk((tmp / "empty").string());
    require(d.ignored.empty(), "empty file");

    // include depth: sixteen nested includes are read, seventeen are refused
    for (int depth : {16, 17}) {
        const fs::path dir = tmp / ("chain" + std::to_string(depth));
        fs::create_directories(dir);
        for (int k = 0; k <= depth; ++k)
            write(dir / ("f" + std::to_string(k)), k < depth ? "minVol " + std::to_string(k) + ";\n#include \"f" + std::to_string(k + 1) + "\"\n"
                                                              : std::string("maxConcave 33;\n"));
        if (depth == 16) {
            d = readOk((dir / "f0").string());
            require(d.value[keyIndex("maxConcave")] == 33 && d.value[keyIndex("minVol")] == 15, "a chain of sixteen includes");
        } else
            readFails((dir / "f0").string(), {"f16:2", "deeper than 16"});
    }
    // an absolute include, and a file that includes itself
    write(tmp / "abs", "#include \"" + fix + "/partial\"\n");
    d = readOk((tmp / "abs").string());
    require(d.value[keyIndex("maxNonOrtho")] == 55, "absolute include");
    write(tmp / "self", "\n#include \"self\"\n");
    readFails((tmp / "self").string(), {"self:2", "include cycle"});

    std::printf("ok %d checks\n", g_checks);
    return 0;
}
