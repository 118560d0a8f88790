// quality_dict.hpp -- reading the limits of an OpenFOAM system/meshQualityDict (DESIGN.md "Mesh quality", 10.18): the one parser
// behind smhost_read_mesh_quality_dict (include/smhost.h) and `smoothMesh -meshQualityDict`.
#pragma once
#include <string>
#include <vector>

namespace smhost {

// the keys that are read, in the order of smhost_read_mesh_quality_dict's arrays
constexpr int kQualityDictKeys = 13;
extern const char* const kQualityDictKeyNames[kQualityDictKeys];

struct MeshQualityDict {
    double value[kQualityDictKeys] = {};
    bool found[kQualityDictKeys] = {};
    std::vector<std::string> ignored;      // every other top-level key, sub-dictionaries included (FoamFile is not), once each
};

// Reads `path`.  Grammar: FoamFile { ... } is skipped; // and /* */ comments; top-level `key value;` entries; sub-dictionaries are
// skipped with brace nesting; #include "file" relative to the including file; #includeEtc "X" as X under each of etcDirs in turn;
// later entries override earlier ones; include depth <= 16.  Throws std::runtime_error("<file>:<line>: ...") for an include cycle,
// a missing file, a $macro, an unterminated brace, comment or string, a missing ';', any other # directive, and a non-numeric or
// NaN value of a key that is read.  No default values are compiled in: a key that no file gives stays !found.
void readMeshQualityDict(const std::string& path, const std::vector<std::string>& etcDirs, MeshQualityDict& out);

}  // namespace smhost
