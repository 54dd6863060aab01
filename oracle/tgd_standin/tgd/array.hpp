/*
 * tgd/array.hpp -- TEST INFRASTRUCTURE: a stand-in for the array container that the reference's
 * headers include, written from the way those headers USE it (constructors from ({w, h}, comps)
 * and from a description, dimension(s), component*, elementCount, data, get<T>(i), get<T>(i, c),
 * operator[], set, and three kinds of tag lists with set / value).  It exists so that
 * oracle/ref_frames.cpp can compile the reference's whole library and run its mcpt(); the
 * product never sees it (include/tgd/ is the product's own container).  Elements are stored
 * interleaved, x fastest; copies share the storage.  No file formats (tgd/io.hpp).
 */
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace TGD {

enum Type { int8, uint8, int16, uint16, int32, uint32, int64, uint64, float32, float64 };

inline size_t typeSize(Type t)
{
    static const size_t sizes[] = { 1, 1, 2, 2, 4, 4, 8, 8, 4, 8 };
    return sizes[t];
}

template<typename T> constexpr Type typeFromTemplate();
template<> constexpr Type typeFromTemplate<int8_t>() { return int8; }
template<> constexpr Type typeFromTemplate<uint8_t>() { return uint8; }
template<> constexpr Type typeFromTemplate<int16_t>() { return int16; }
template<> constexpr Type typeFromTemplate<uint16_t>() { return uint16; }
template<> constexpr Type typeFromTemplate<int32_t>() { return int32; }
template<> constexpr Type typeFromTemplate<uint32_t>() { return uint32; }
template<> constexpr Type typeFromTemplate<int64_t>() { return int64; }
template<> constexpr Type typeFromTemplate<uint64_t>() { return uint64; }
template<> constexpr Type typeFromTemplate<float>() { return float32; }
template<> constexpr Type typeFromTemplate<double>() { return float64; }

class TagList
{
    std::map<std::string, std::string> _tags;

public:
    void set(const std::string& key, const std::string& value) { _tags[key] = value; }
    bool contains(const std::string& key) const { return _tags.count(key) != 0; }
    std::string value(const std::string& key, const std::string& fallback = std::string()) const
    {
        auto it = _tags.find(key);
        return it == _tags.end() ? fallback : it->second;
    }
};

class ArrayDescription
{
protected:
    std::vector<size_t> _dims;
    size_t _comps = 0;
    Type _type = uint8;
    TagList _globalTags;
    std::vector<TagList> _dimTags, _compTags;

public:
    ArrayDescription() {}
    ArrayDescription(const std::vector<size_t>& dims, size_t comps, Type type) :
        _dims(dims), _comps(comps), _type(type), _dimTags(dims.size()), _compTags(comps)
    {
    }

    size_t dimensionCount() const { return _dims.size(); }
    size_t dimension(size_t d) const { return _dims[d]; }
    const std::vector<size_t>& dimensions() const { return _dims; }
    size_t componentCount() const { return _comps; }
    Type componentType() const { return _type; }
    size_t componentSize() const { return typeSize(_type); }
    size_t elementSize() const { return _comps * componentSize(); }
    size_t elementCount() const
    {
        if (_dims.empty())
            return 0;
        size_t n = 1;
        for (size_t d : _dims)
            n *= d;
        return n;
    }
    size_t dataSize() const { return elementCount() * elementSize(); }
    const ArrayDescription& description() const { return *this; }

    TagList& globalTagList() { return _globalTags; }
    const TagList& globalTagList() const { return _globalTags; }
    TagList& dimensionTagList(size_t d) { return _dimTags[d]; }
    const TagList& dimensionTagList(size_t d) const { return _dimTags[d]; }
    TagList& componentTagList(size_t c) { return _compTags[c]; }
    const TagList& componentTagList(size_t c) const { return _compTags[c]; }
};

class ArrayContainer : public ArrayDescription
{
    std::shared_ptr<std::vector<unsigned char>> _data;

    size_t linear(const std::vector<size_t>& index) const
    {
        size_t i = 0, stride = 1;
        for (size_t d = 0; d < _dims.size(); d++) {
            i += index[d] * stride;
            stride *= _dims[d];
        }
        return i;
    }

public:
    ArrayContainer() {}
    ArrayContainer(const ArrayDescription& desc) : ArrayDescription(desc), _data(new std::vector<unsigned char>(desc.dataSize(), 0)) {}
    ArrayContainer(const std::vector<size_t>& dims, size_t comps, Type type) : ArrayContainer(ArrayDescription(dims, comps, type)) {}

    void* data() { return _data ? _data->data() : nullptr; }
    const void* data() const { return _data ? _data->data() : nullptr; }

    void* get(size_t i) { return _data->data() + i * elementSize(); }
    const void* get(size_t i) const { return _data->data() + i * elementSize(); }
    void* get(const std::vector<size_t>& index) { return get(linear(index)); }
    const void* get(const std::vector<size_t>& index) const { return get(linear(index)); }

    template<typename T> T* get(size_t i) { return static_cast<T*>(get(i)); }
    template<typename T> const T* get(size_t i) const { return static_cast<const T*>(get(i)); }
    template<typename T> T* get(const std::vector<size_t>& index) { return static_cast<T*>(get(index)); }
    template<typename T> const T* get(const std::vector<size_t>& index) const { return static_cast<const T*>(get(index)); }
    template<typename T> T get(size_t i, size_t c) const { return get<T>(i)[c]; }
    template<typename T> T get(const std::vector<size_t>& index, size_t c) const { return get<T>(index)[c]; }

    template<typename T> void set(size_t i, size_t c, T v) { get<T>(i)[c] = v; }
    template<typename T> void set(const std::vector<size_t>& index, size_t c, T v) { get<T>(index)[c] = v; }
    template<typename T> void set(size_t i, const std::vector<T>& v)
    {
        for (size_t c = 0; c < v.size() && c < _comps; c++)
            get<T>(i)[c] = v[c];
    }
    template<typename T> void set(const std::vector<size_t>& index, const std::vector<T>& v) { set<T>(linear(index), v); }

    ArrayContainer deepCopy() const
    {
        ArrayContainer r(description());
        if (dataSize() > 0)
            std::memcpy(r.data(), data(), dataSize());
        return r;
    }
};

template<typename T> class Array : public ArrayContainer
{
public:
    Array() {}
    Array(const ArrayDescription& desc) : ArrayContainer(ArrayDescription(desc.dimensions(), desc.componentCount(), typeFromTemplate<T>()))
    {
        globalTagList() = desc.globalTagList();
    }
    Array(const std::vector<size_t>& dims, size_t comps) : ArrayContainer(dims, comps, typeFromTemplate<T>()) {}
    Array(std::initializer_list<size_t> dims, size_t comps) : ArrayContainer(std::vector<size_t>(dims), comps, typeFromTemplate<T>()) {}
    /* a container whose components already have this type shares its storage; any other gives an empty array */
    Array(const ArrayContainer& container) : ArrayContainer(container.componentType() == typeFromTemplate<T>() ? container : ArrayContainer())
    {
    }

    T* operator[](size_t i) { return ArrayContainer::get<T>(i); }
    const T* operator[](size_t i) const { return ArrayContainer::get<T>(i); }
    T* operator[](const std::vector<size_t>& index) { return ArrayContainer::get<T>(index); }
    const T* operator[](const std::vector<size_t>& index) const { return ArrayContainer::get<T>(index); }

    /* the container's accessors, with this array's type where the caller names none */
    template<typename U = T> U* get(size_t i) { return ArrayContainer::get<U>(i); }
    template<typename U = T> const U* get(size_t i) const { return ArrayContainer::get<U>(i); }
    template<typename U = T> U* get(const std::vector<size_t>& index) { return ArrayContainer::get<U>(index); }
    template<typename U = T> const U* get(const std::vector<size_t>& index) const { return ArrayContainer::get<U>(index); }
    template<typename U = T> U get(size_t i, size_t c) const { return ArrayContainer::get<U>(i, c); }
    template<typename U = T> U get(const std::vector<size_t>& index, size_t c) const { return ArrayContainer::get<U>(index, c); }
    template<typename U = T> void set(size_t i, size_t c, U v) { ArrayContainer::set<U>(i, c, v); }
    template<typename U = T> void set(const std::vector<size_t>& index, size_t c, U v) { ArrayContainer::set<U>(index, c, v); }
    template<typename U = T> void set(size_t i, const std::vector<U>& v) { ArrayContainer::set<U>(i, v); }
    template<typename U = T> void set(const std::vector<size_t>& index, const std::vector<U>& v) { ArrayContainer::set<U>(index, v); }
};

}
