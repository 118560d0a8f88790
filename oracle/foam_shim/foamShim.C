// foamShim.C -- the definitions behind foamShim.H.  TEST INFRASTRUCTURE ONLY; included once, by oracle/ref_driver.cpp.
#include "foamShim.H"

namespace Foam
{
namespace shim
{
MeshInput& meshInput() { static MeshInput m; return m; }
Recorder& recorder() { static Recorder r; return r; }
const Time*& currentTime() { static const Time* t = nullptr; return t; }
static std::ostringstream& infoBuffer() { static std::ostringstream s; return s; }
static std::ostringstream& errorBuffer() { static std::ostringstream s; return s; }
}

std::ostream& Ostream::stream()
{
    if (!os_) os_ = (static_cast<void*>(this) == static_cast<void*>(&FatalError)) ? &shim::errorBuffer() : &shim::infoBuffer();
    return *os_;
}
Ostream Info;
Ostream Pout;
error FatalError;
Ostream& operator<<(Ostream& os, const errorManip&)
{
    const std::string text = shim::errorBuffer().str();
    shim::errorBuffer().str("");
    throw shim::FatalException(text);
    return os;
}

word Time::controlDictName("controlDict");
word Time::timeName(scalar v)
{
    std::ostringstream buf;
    buf.precision(6);
    buf << v;
    return word(buf.str());
}
instant::instant(scalar v) : value(v), name(Time::timeName(v)) {}

argList::argList(int& argc, char**& argv)
{
    for (int i = 1; i < argc; ++i)
    {
        const std::string a(argv[i]);
        if (a.size() < 2 || a[0] != '-') shim::fail("foam_shim: unexpected argument '" + a + "'");
        const std::string name = a.substr(1);
        if (name == "parallel") shim::fail("foam_shim: the stand-in runs in serial only");
        std::map<std::string, bool>::const_iterator it = valid_().find(name);
        if (it == valid_().end() && name != "case") shim::fail("Invalid option: -" + name);
        if (name == "case" || it->second)
        {
            if (i + 1 >= argc) shim::fail("Option -" + name + " requires an argument");
            options_[name] = argv[++i];
        }
        else options_[name] = "";
    }
}

wordReList::wordReList(Istream& is)
{
    const std::string& s = is.text;
    size_t i = 0;
    const size_t n = s.size();
    bool inList = false, closed = false;
    while (i < n)
    {
        const char c = s[i];
        if (c == ' ' || c == '\t' || c == '\n') { ++i; continue; }
        if (c == '(' && !inList && size() == 0) { inList = true; ++i; continue; }
        if (c == ')' && inList) { closed = true; ++i; break; }
        if (c == '"')
        {
            const size_t e = s.find('"', i + 1);
            if (e == std::string::npos) shim::fail("foam_shim: unterminated string in '" + s + "'");
            append(wordRe(s.substr(i + 1, e - i - 1), true));
            i = e + 1;
        }
        else
        {
            size_t e = i;
            while (e < n && s[e] != ' ' && s[e] != '\t' && s[e] != '\n' && s[e] != ')' && s[e] != '(' && s[e] != '"') ++e;
            append(wordRe(s.substr(i, e - i), false));
            i = e;
        }
        if (!inList) break;
    }
    if (inList && !closed) shim::fail("foam_shim: list without closing bracket in '" + s + "'");
}

labelHashSet polyBoundaryMesh::patchSet(const wordReList& l) const
{
    labelHashSet set;
    for (label k = 0; k < l.size(); ++k)
        for (label p = 0; p < size(); ++p)
            if (l[k].match((*this)[p].name())) set.insert(p);
    return set;
}

static void fill(labelListList& dst, const std::vector<std::vector<label> >& src, label rows, const char* what)
{
    if (label(src.size()) != rows) shim::fail(std::string("foam_shim: addressing '") + what + "' was not handed over, or has the wrong number of rows");
    dst.setSize(rows);
    for (label i = 0; i < rows; ++i)
    {
        dst[i].setSize(label(src[size_t(i)].size()));
        for (label j = 0; j < dst[i].size(); ++j) dst[i][j] = src[size_t(i)][size_t(j)];
    }
}

polyMesh::polyMesh() : instance_("constant")
{
    const shim::MeshInput& in = shim::meshInput();
    if (in.nPoints <= 0 || !in.geometry) shim::fail("foam_shim: no mesh was handed over");
    points_.setSize(in.nPoints);
    for (label i = 0; i < in.nPoints; ++i) points_[i] = point(in.points[3 * size_t(i)], in.points[3 * size_t(i) + 1], in.points[3 * size_t(i) + 2]);
    faces_.setSize(in.nFaces);
    for (label f = 0; f < in.nFaces; ++f)
    {
        faces_[f].setSize(label(in.faces[size_t(f)].size()));
        for (label j = 0; j < faces_[f].size(); ++j) faces_[f][j] = in.faces[size_t(f)][size_t(j)];
    }
    owner_.setSize(in.nInternalFaces);
    neighbour_.setSize(in.nInternalFaces);
    for (label f = 0; f < in.nInternalFaces; ++f) { owner_[f] = in.owner[size_t(f)]; neighbour_[f] = in.neighbour[size_t(f)]; }
    edges_.setSize(in.nEdges);
    for (label e = 0; e < in.nEdges; ++e) edges_[e] = edge(in.edges[2 * size_t(e)], in.edges[2 * size_t(e) + 1]);
    std::map<std::string, std::vector<std::vector<label> > > a = in.addressing;
    fill(pointCells_, a["pointCells"], in.nPoints, "pointCells");
    fill(pointPoints_, a["pointPoints"], in.nPoints, "pointPoints");
    fill(pointFaces_, a["pointFaces"], in.nPoints, "pointFaces");
    fill(pointEdges_, a["pointEdges"], in.nPoints, "pointEdges");
    fill(edgeFaces_, a["edgeFaces"], in.nEdges, "edgeFaces");
    fill(edgeCells_, a["edgeCells"], in.nEdges, "edgeCells");
    fill(cellPoints_, a["cellPoints"], in.nCells, "cellPoints");
    faceCentres_.setSize(in.nFaces);
    faceAreas_.setSize(in.nFaces);
    cellCentres_.setSize(in.nCells);
    for (size_t p = 0; p < in.patchName.size(); ++p)
    {
        polyPatch* pp = in.patchKind[p] == 1 ? new processorPolyPatch : in.patchKind[p] == 2 ? new emptyPolyPatch : new polyPatch;
        pp->name_ = word(in.patchName[p]);
        pp->start_ = in.patchStart[p];
        pp->size_ = in.patchSize[p];
        if (pp->start_ < in.nInternalFaces || pp->start_ + pp->size_ > in.nFaces) { delete pp; shim::fail("foam_shim: patch face range outside the boundary faces"); }
        pp->faceCells_.setSize(pp->size_);
        for (label i = 0; i < pp->size_; ++i) pp->faceCells_[i] = in.owner[size_t(pp->start_ + i)];
        boundaryMesh_.patches_.push_back(std::unique_ptr<polyPatch>(pp));
        fvPatch fp;
        fp.start_ = pp->start_;
        fp.size_ = pp->size_;
        boundary_.patches_.push_back(fp);
    }
    updateGeometry();
}

void polyMesh::updateGeometry()
{
    const shim::MeshInput& in = shim::meshInput();
    const size_t nP = size_t(nPoints()), nF = size_t(nFaces()), nC = size_t(nCells());
    std::vector<double> p(3 * nP), fc(3 * nF), fa(3 * nF), cc(3 * nC);
    for (size_t i = 0; i < nP; ++i) for (int k = 0; k < 3; ++k) p[3 * i + size_t(k)] = points_[label(i)][k];
    in.geometry(p.data(), fc.data(), fa.data(), cc.data(), in.geometryUser);
    for (size_t i = 0; i < nF; ++i)
    {
        faceCentres_[label(i)] = vector(fc[3 * i], fc[3 * i + 1], fc[3 * i + 2]);
        faceAreas_[label(i)] = vector(fa[3 * i], fa[3 * i + 1], fa[3 * i + 2]);
    }
    for (size_t i = 0; i < nC; ++i) cellCentres_[label(i)] = vector(cc[3 * i], cc[3 * i + 1], cc[3 * i + 2]);
    for (size_t k = 0; k < boundary_.patches_.size(); ++k)
    {
        fvPatch& fp = boundary_.patches_[k];
        fp.Cf_.setSize(fp.size_);
        fp.Sf_.setSize(fp.size_);
        fp.magSf_.setSize(fp.size_);
        for (label i = 0; i < fp.size_; ++i)
        {
            fp.Cf_[i] = faceCentres_[fp.start_ + i];
            fp.Sf_[i] = faceAreas_[fp.start_ + i];
            fp.magSf_[i] = mag(fp.Sf_[i]);
        }
    }
}

static std::vector<double> flat(const pointField& p)
{
    std::vector<double> v(3 * size_t(p.size()));
    for (label i = 0; i < p.size(); ++i) for (int k = 0; k < 3; ++k) v[3 * size_t(i) + size_t(k)] = p[i][k];
    return v;
}
void fvMesh::movePoints(const pointField& p)
{
    if (p.size() != points_.size()) shim::fail("foam_shim: movePoints with a field of the wrong size");
    points_ = p;
    updateGeometry();
    shim::recorder().moved.push_back(flat(points_));
}
bool fvMesh::write() const
{
    shim::recorder().writeName.push_back(shim::currentTime() ? std::string(shim::currentTime()->name()) : std::string("?"));
    shim::recorder().written.push_back(flat(points_));
    return true;
}
}  // namespace Foam
