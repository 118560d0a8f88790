// quality_dict.cpp -- the meshQualityDict reader (quality_dict.hpp).  Plain C++17, no GPU.
#include "quality_dict.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace smhost {

const char* const kQualityDictKeyNames[kQualityDictKeys] = {"maxNonOrtho", "maxBoundarySkewness", "maxInternalSkewness", "maxConcave", "minFlatness",
                                                            "minVol", "minTetQuality", "minArea", "minTwist", "minDeterminant",
                                                            "minFaceWeight", "minVolRatio", "minTriangleTwist"};

namespace {

namespace fs = std::filesystem;
constexpr int kMaxIncludeDepth = 16;

[[noreturn]] void failAt(const std::string& file, int line, const std::string& msg) {
    throw std::runtime_error(file + ":" + std::to_string(line) + ": " + msg);
}

struct Token {
    enum Kind { End, Word, String, Open, Close, Semi } kind = End;
    std::string text;
    int line = 0;
};

// the tokens of one file: comments and white space dropped, lines counted from 1
class Lexer {
    const std::string& file;
    const std::string& s;
    size_t i = 0;
    int line = 1;

  public:
    Lexer(const std::string& fileName, const std::string& text) : file(fileName), s(text) {}
    Token next() {
        for (;;) {   // white space and comments
            while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\r' || s[i] == '\n' || s[i] == '\f' || s[i] == '\v')) {
                if (s[i] == '\n') ++line;
                ++i;
            }
            if (i + 1 < s.size() && s[i] == '/' && s[i + 1] == '/') {
                while (i < s.size() && s[i] != '\n') ++i;
                continue;
            }
            if (i + 1 < s.size() && s[i] == '/' && s[i + 1] == '*') {
                const int start = line;
                i += 2;
                for (;;) {
                    if (i + 1 >= s.size()) failAt(file, start, "unterminated /* comment");
                    if (s[i] == '*' && s[i + 1] == '/') { i += 2; break; }
                    if (s[i] == '\n') ++line;
                    ++i;
                }
                continue;
            }
            break;
        }
        Token t;
        t.line = line;
        if (i >= s.size()) return t;
        const char c = s[i];
        if (c == '{' || c == '}' || c == ';') {
            t.kind = c == '{' ? Token::Open : c == '}' ? Token::Close : Token::Semi;
            t.text = std::string(1, c);
            ++i;
            return t;
        }
        if (c == '"') {
            t.kind = Token::String;
            ++i;
            while (i < s.size() && s[i] != '"' && s[i] != '\n') {
                if (s[i] == '\\' && i + 1 < s.size() && s[i + 1] != '\n') ++i;
                t.text += s[i++];
            }
            if (i >= s.size() || s[i] != '"') failAt(file, t.line, "unterminated string");
            ++i;
            return t;
        }
        t.kind = Token::Word;
        while (i < s.size()) {
            const char d = s[i];
            if (d == ' ' || d == '\t' || d == '\r' || d == '\n' || d == '\f' || d == '\v' || d == '{' || d == '}' || d == ';' || d == '"') break;
            if (d == '/' && i + 1 < s.size() && (s[i + 1] == '/' || s[i + 1] == '*')) break;
            t.text += d;
            ++i;
        }
        return t;
    }
};

std::string canonical(const std::string& p) {
    std::error_code ec;
    const fs::path c = fs::weakly_canonical(fs::path(p), ec);
    return ec ? p : c.string();
}

bool isFile(const std::string& p) {
    std::error_code ec;
    return fs::is_regular_file(fs::path(p), ec);
}

struct Reader {
    const std::vector<std::string>& etcDirs;
    MeshQualityDict& out;
    std::vector<std::string> stack;   // the canonical paths of the files being read, outermost first

    void remember(const std::string& key) {
        if (std::find(out.ignored.begin(), out.ignored.end(), key) == out.ignored.end()) out.ignored.push_back(key);
    }

    // behind an Open token at openLine: everything up to the matching Close
    void skipBlock(Lexer& lx, const std::string& file, int openLine) {
        for (int depth = 1; depth > 0;) {
            const Token t = lx.next();
            if (t.kind == Token::End) failAt(file, openLine, "unterminated {");
            if (t.kind == Token::Open) ++depth;
            if (t.kind == Token::Close) --depth;
        }
    }

    void readFile(const std::string& path, const std::string& fromFile, int fromLine) {
        if (!isFile(path)) {
            if (fromFile.empty()) throw std::runtime_error(path + ":0: cannot read the file");
            failAt(fromFile, fromLine, "cannot read the included file " + path);
        }
        const std::string canon = canonical(path);
        if (std::find(stack.begin(), stack.end(), canon) != stack.end()) failAt(fromFile, fromLine, "include cycle: " + path + " is being read already");
        if ((int)stack.size() > kMaxIncludeDepth) failAt(fromFile, fromLine, "includes nested deeper than " + std::to_string(kMaxIncludeDepth));
        std::ifstream in(path, std::ios::binary);
        if (!in) failAt(fromFile.empty() ? path : fromFile, fromLine, "cannot read the file " + path);
        std::ostringstream buf;
        buf << in.rdbuf();
        const std::string text = buf.str();
        stack.push_back(canon);
        parse(path, text);
        stack.pop_back();
    }

    void parse(const std::string& file, const std::string& text) {
        Lexer lx(file, text);
        for (;;) {
            const Token key = lx.next();
            if (key.kind == Token::End) return;
            if (key.kind == Token::Close) failAt(file, key.line, "} without {");
            if (key.kind == Token::Open) failAt(file, key.line, "{ without a name");
            if (key.kind == Token::Semi) continue;
            if (key.kind == Token::String) failAt(file, key.line, "a string where a keyword is expected: \"" + key.text + "\"");
            if (key.text[0] == '$') failAt(file, key.line, "macro " + key.text + ": macros are not expanded");
            if (key.text[0] == '#') {
                directive(lx, file, key);
                continue;
            }
            // the entry: a sub-dictionary, or the value's tokens up to the ';'
            std::vector<Token> value;
            for (;;) {
                const Token t = lx.next();
                if (t.kind == Token::Semi) break;
                if (t.kind == Token::Open && value.empty()) {
                    skipBlock(lx, file, t.line);
                    if (key.text != "FoamFile") remember(key.text);
                    value.clear();
                    value.push_back(t);   // (marks the entry as a block)
                    break;
                }
                if (t.kind == Token::End || t.kind == Token::Open || t.kind == Token::Close || t.line != key.line)
                    failAt(file, key.line, "missing ; behind the entry " + key.text);
                if (t.kind == Token::Word && t.text[0] == '$') failAt(file, t.line, "macro " + t.text + ": macros are not expanded");
                if (t.kind == Token::Word && t.text[0] == '#') failAt(file, t.line, "directive " + t.text + " inside the entry " + key.text);
                value.push_back(t);
            }
            if (!value.empty() && value[0].kind == Token::Open) continue;
            const char* const* names = kQualityDictKeyNames;
            const char* const* hit = std::find_if(names, names + kQualityDictKeys, [&](const char* n) { return key.text == n; });
            if (hit == names + kQualityDictKeys) {
                remember(key.text);
                continue;
            }
            if (value.size() != 1 || value[0].kind != Token::Word) failAt(file, key.line, key.text + " wants one number");
            const std::string& v = value[0].text;
            char* end = nullptr;
            const double x = std::strtod(v.c_str(), &end);
            if (end == v.c_str() || *end != '\0') failAt(file, key.line, key.text + ": '" + v + "' is not a number");
            if (std::isnan(x)) failAt(file, key.line, key.text + " is NaN");
            out.value[hit - names] = x;
            out.found[hit - names] = true;
        }
    }

    void directive(Lexer& lx, const std::string& file, const Token& d) {
        if (d.text != "#include" && d.text != "#includeEtc") failAt(file, d.line, "directive " + d.text + " is not supported");
        const Token name = lx.next();
        if (name.kind != Token::String || name.line != d.line) failAt(file, d.line, d.text + " wants a quoted file name");
        if (name.text.find('$') != std::string::npos) failAt(file, d.line, "macro in " + d.text + " \"" + name.text + "\": macros are not expanded");
        if (d.text == "#include") {
            const fs::path p(name.text);
            readFile(p.is_absolute() ? p.string() : (fs::path(file).parent_path() / p).string(), file, d.line);
            return;
        }
        std::string tried;
        for (const std::string& dir : etcDirs) {
            const std::string p = (fs::path(dir) / name.text).string();
            if (isFile(p)) {
                readFile(p, file, d.line);
                return;
            }
            tried += (tried.empty() ? "" : ", ") + dir;
        }
        failAt(file, d.line, "#includeEtc \"" + name.text + "\": not found under " + (tried.empty() ? "any directory (none was given)" : tried));
    }
};

}  // namespace

void readMeshQualityDict(const std::string& path, const std::vector<std::string>& etcDirs, MeshQualityDict& out) {
    out = MeshQualityDict{};
    Reader r{etcDirs, out, {}};
    r.readFile(path, "", 0);
}

}  // namespace smhost
