classdef binauralDecodeStream < handle
% binauralDecode a block at a time on the GPU, for a listener whose head moves while the sound plays (DESIGN.md section 9.3).
%   s = binauralDecodeStream(decodingFilterLeft, decodingFilterRight, blockSize, shDefinition, rotationDomain, complexInput, encoder)
%   out = s.push(block, horRotAngleRad, pitchRad, rollRad, setIndex)    block [k*blockSize x numChannels] -> out [k*blockSize x 2]
%   s.reset()    zero history        delete(s)    releases the device memory
% Concatenating the pushed blocks into x and the angles per sample, the concatenated outputs equal
% binauralDecode(x, fs, wL, wR, fs, false, [], [], yaw, shDefinition, rotationDomain, pitch, roll) to rounding: no delay cut, no
% resampling; a dry source signal goes through a sourceFieldStream first.  blockSize: a power of two from 64 to 2048.  Each angle: [] (0), a scalar (constant over the push)
% or one value per sample.  For complex signals or filters the output is the real part; the discarded sum is not reported.
% A bank of filter sets (DESIGN.md section 9.4): filters [len x numChannels x numSets] make a stream of numSets sets (s.numSets), and
% setIndex chooses the set per block, ONE-based as MATLAB counts: [] (every block keeps the set of the block before it; set 1 on a
% fresh stream), a scalar (every block of this push) or one index per block.  A change of set is cross-faded over the block that
% changes (sample i of it goes to the new set with the gain i / blockSize, i = 1 .. blockSize, and to the old one with the rest);
% the first block after creation or reset does not fade; a constant index gives the plain stream on that set bit for bit.
% An encoder (DESIGN.md section 9.6): with encoder [numChannels x numMics], e.g. pinv(getSH(order, micGrid).').', the stream is pushed
% blocks of REAL microphone signals [k*blockSize x numMics] and returns what the plain stream returns for block * encoder.', the
% encoder running inside the rotation launch.  1 <= numMics, numChannels <= 64.
    properties (SetAccess = private)
        handle = 0
        blockSize
        numSets
    end
    methods
        function s = binauralDecodeStream(decodingFilterLeft, decodingFilterRight, blockSize, shDefinition, rotationDomain, complexInput, encoder)
            if nargin < 4; shDefinition = 'real'; end
            if nargin < 5; rotationDomain = 'sh'; end
            if nargin < 6; complexInput = false; end
            if nargin < 7; encoder = []; end
            if isreal(decodingFilterLeft) ~= isreal(decodingFilterRight)
                decodingFilterLeft = complex(decodingFilterLeft); decodingFilterRight = complex(decodingFilterRight);
            end
            s.blockSize = blockSize;
            s.numSets = size(decodingFilterLeft, 3);
            s.handle = emagls_mex('stream_create', double(decodingFilterLeft), double(decodingFilterRight), double(blockSize), ...
                                  shDefinition, rotationDomain, logical(complexInput), double(encoder));
        end
        function out = push(s, block, horRotAngleRad, pitchRad, rollRad, setIndex)
            if nargin < 3; horRotAngleRad = []; end
            if nargin < 4; pitchRad = []; end
            if nargin < 5; rollRad = []; end
            if nargin < 6; setIndex = []; end
            out = emagls_mex('stream_push', s.handle, double(block), double(horRotAngleRad), double(pitchRad), double(rollRad), ...
                             double(setIndex));
        end
        function reset(s)
            emagls_mex('stream_reset', s.handle);
        end
        function delete(s)
            if s.handle > 0
                emagls_mex('stream_destroy', s.handle);
                s.handle = 0;
            end
        end
    end
end
