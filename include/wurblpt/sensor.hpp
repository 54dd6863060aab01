/*
 * sensor.hpp -- the film (reference sensor.hpp:36-82, sensor_rgb.hpp:35-98).
 * accumulateRadiance()/finishPixel() run in the HIP kernel; SensorRGB holds the frame,
 * float[height][width][3] with row 0 at the bottom, and the four gate values.
 */
#pragma once

#include <cmath>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "array.hpp"

namespace WurblPT {

class Material;

class Sensor
{
public:
    constexpr static int maxPixelComponents = 3;
    virtual ~Sensor() {}
    virtual unsigned int width() const { return 0; }
    virtual unsigned int height() const { return 0; }
    virtual ArrayContainer* pixelArray() { return nullptr; }
    virtual float aspectRatio() const { return float(width()) / height(); }
};

class SensorRGB final : public Sensor
{
private:
    Array<float> _frame;

public:
    const float minDistToLight, maxDistToLight;
    const float minPathLen, maxPathLen;

    SensorRGB(unsigned int width, unsigned int height, float minDistToLight = 0.0f,
            float maxDistToLight = std::numeric_limits<float>::max(), float minPathLen = 0.0f,
            float maxPathLen = std::numeric_limits<float>::max()) :
        _frame(width, height, 3), minDistToLight(minDistToLight), maxDistToLight(maxDistToLight), minPathLen(minPathLen),
        maxPathLen(maxPathLen)
    {
    }
    virtual unsigned int width() const override { return _frame.dimension(0); }
    virtual unsigned int height() const override { return _frame.dimension(1); }
    virtual ArrayContainer* pixelArray() override { return &_frame; }
    const Array<float>& result() const { return _frame; }
};

/* A transient film (light-in-flight rendering; a capability of this port, not of the reference): mcpt() renders the
 * all-light frame and binCount() frames in one pass.  Bin k holds the light whose optical path length lies in
 * [binEdges()[k], binEdges()[k + 1]), per channel, behind the distance-to-light gate; bin k is bit-identical to a SensorRGB
 * render with minPathLen = edge k and maxPathLen = nextafterf(edge k + 1, -inf).  result() is the frame with the distance
 * gate only.  The bins cost binCount() * width * height * 12 bytes. */
class SensorRGBTransient final : public Sensor
{
private:
    Array<float> _frame;
    std::vector<float> _edges;
    std::vector<Array<float>> _bins;

    void init(unsigned int width, unsigned int height)
    {
        if (_edges.size() < 2)
            throw std::invalid_argument("SensorRGBTransient: at least one bin");
        for (size_t k = 0; k < _edges.size(); k++) {
            const float e = _edges[k];
            if (std::isnan(e) || (std::isinf(e) && !(k + 1 == _edges.size() && e > 0.0f)))
                throw std::invalid_argument("SensorRGBTransient: bin edge " + std::to_string(k) + " is not finite (only the last may be +inf)");
            if (k > 0 && !(e > _edges[k - 1]))
                throw std::invalid_argument("SensorRGBTransient: bin edges must increase (edge " + std::to_string(k) + ")");
        }
        _bins.reserve(_edges.size() - 1);
        for (size_t k = 0; k + 1 < _edges.size(); k++)
            _bins.emplace_back(width, height, 3);
    }

public:
    const float minDistToLight, maxDistToLight;

    /* binCount bins of width binWidth from minPathLen: edge k = minPathLen + (float)k * binWidth, two float roundings */
    SensorRGBTransient(unsigned int width, unsigned int height, float minPathLen, float binWidth, unsigned int binCount,
            float minDistToLight = 0.0f, float maxDistToLight = std::numeric_limits<float>::max()) :
        _frame(width, height, 3), minDistToLight(minDistToLight), maxDistToLight(maxDistToLight)
    {
        _edges.resize(size_t(binCount) + 1);
        for (unsigned int k = 0; k <= binCount; k++) {
            volatile float step = float(k) * binWidth; /* rounded on its own: no fused multiply-add */
            _edges[k] = minPathLen + step;
        }
        init(width, height);
    }
    /* explicit edges: binCount + 1 increasing floats, all finite except that the last may be +inf */
    SensorRGBTransient(unsigned int width, unsigned int height, const std::vector<float>& edges,
            float minDistToLight = 0.0f, float maxDistToLight = std::numeric_limits<float>::max()) :
        _frame(width, height, 3), _edges(edges), minDistToLight(minDistToLight), maxDistToLight(maxDistToLight)
    {
        init(width, height);
    }
    virtual unsigned int width() const override { return _frame.dimension(0); }
    virtual unsigned int height() const override { return _frame.dimension(1); }
    virtual ArrayContainer* pixelArray() override { return &_frame; }
    unsigned int binCount() const { return _edges.size() - 1; }
    const std::vector<float>& binEdges() const { return _edges; }
    const Array<float>& result() const { return _frame; }
    const Array<float>& bin(unsigned int k) const { return _bins.at(k); }
    Array<float>& bin(unsigned int k) { return _bins.at(k); }
};

/* Light groups (a capability of this port, not of the reference): mcpt() renders the frame and groupCount() frames in one
 * pass, group(g) holding the light of the emitters assigned to group g.  Nothing that steers a path reads an emitted radiance,
 * so group(g) is bit-identical to a SensorRGB render of the scene in which only group g's emitters emit; both gates apply to the
 * groups as to the frame.  assign() takes the Material an emitting hitable was given (a MaterialTwoSided assigns both its
 * children, unless a child has an assignment of its own); emitters that were not assigned, and the environment unless
 * assignEnvironment() says otherwise, go to group 0.
 * mixLightGroups() (postproc.hpp) weights the groups into one frame afterwards.  The groups cost groupCount() * width *
 * height * 12 bytes. */
class SensorRGBLightGroups final : public Sensor
{
private:
    Array<float> _frame;
    std::vector<Array<float>> _groups;
    std::map<const Material*, unsigned int> _groupOf;
    unsigned int _envGroup;

public:
    constexpr static unsigned int maxGroups = 255; /* WPT_LIGHT_GROUPS_MAX */
    const float minDistToLight, maxDistToLight;
    const float minPathLen, maxPathLen;

    SensorRGBLightGroups(unsigned int width, unsigned int height, unsigned int groupCount, float minDistToLight = 0.0f,
            float maxDistToLight = std::numeric_limits<float>::max(), float minPathLen = 0.0f,
            float maxPathLen = std::numeric_limits<float>::max()) :
        _frame(width, height, 3), _envGroup(0), minDistToLight(minDistToLight), maxDistToLight(maxDistToLight), minPathLen(minPathLen),
        maxPathLen(maxPathLen)
    {
        if (groupCount < 1 || groupCount > maxGroups)
            throw std::invalid_argument("SensorRGBLightGroups: 1 to " + std::to_string(maxGroups) + " groups");
        _groups.reserve(groupCount);
        for (unsigned int g = 0; g < groupCount; g++)
            _groups.emplace_back(width, height, 3);
    }
    void assign(const Material* material, unsigned int g)
    {
        if (!material || g >= groupCount())
            throw std::invalid_argument("SensorRGBLightGroups: group " + std::to_string(g) + " of " + std::to_string(groupCount()));
        _groupOf[material] = g;
    }
    void assignEnvironment(unsigned int g)
    {
        if (g >= groupCount())
            throw std::invalid_argument("SensorRGBLightGroups: group " + std::to_string(g) + " of " + std::to_string(groupCount()));
        _envGroup = g;
    }
    virtual unsigned int width() const override { return _frame.dimension(0); }
    virtual unsigned int height() const override { return _frame.dimension(1); }
    virtual ArrayContainer* pixelArray() override { return &_frame; }
    unsigned int groupCount() const { return _groups.size(); }
    unsigned int environmentGroup() const { return _envGroup; }
    const std::map<const Material*, unsigned int>& assignments() const { return _groupOf; }
    const Array<float>& result() const { return _frame; }
    const Array<float>& group(unsigned int g) const { return _groups.at(g); }
    Array<float>& group(unsigned int g) { return _groups.at(g); }
};

}
