/*
 * tgd/io.hpp -- TEST INFRASTRUCTURE: the file functions that the reference's headers name, as
 * stubs that fail.  See tgd/array.hpp next to this file.  No file format is read or written:
 * load() returns an empty array and reports a failure, save() reports a failure.
 */
#pragma once

#include <string>

#include "array.hpp"

namespace TGD {

enum Error { ErrorNone = 0, ErrorFeaturesUnsupported = 1 };

inline const char* strerror(Error e)
{
    return e == ErrorNone ? "success" : "the stand-in container has no file formats";
}

inline ArrayContainer load(const std::string&, const TagList& = TagList(), Error* error = nullptr)
{
    if (error)
        *error = ErrorFeaturesUnsupported;
    return ArrayContainer();
}

inline Error save(const ArrayContainer&, const std::string&, const TagList& = TagList())
{
    return ErrorFeaturesUnsupported;
}

}
