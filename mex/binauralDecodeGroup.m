classdef binauralDecodeGroup < handle
% Many listeners of one sound field in one push on the GPU (DESIGN.md section 9.5): one bank of filter sets, stored once, and
% numListeners listeners, each with the state a binauralDecodeStream has.
%   g = binauralDecodeGroup(decodingFilterLeft, decodingFilterRight, blockSize, numListeners, shDefinition, rotationDomain, complexInput, encoder)
%   out = g.push(block, horRotAngleRad, pitchRad, rollRad, setIndex)    block [k*blockSize x numChannels], the common signal
%   g.reset()  every listener back to zero history     g.reset(l)  listener l alone (who joins)     delete(g)
% Listeners run along the LAST dimension: out [k*blockSize x 2 x numListeners]; each angle [] (0), [1 x numListeners] (constant
% over the push) or [k*blockSize x numListeners]; setIndex ONE-based, [] (every listener keeps their set; set 1 on a fresh
% listener), [1 x numListeners] or [k x numListeners].  out(:, :, l) is, bit for bit, what a binauralDecodeStream of the same
% filters returns when it is fed the same blocks with listener l's angles and indices; a block costs at most three kernel
% launches for the whole group.  The push takes the yaw rule when no listener has a pitch or a roll; otherwise every listener
% goes through the three-axis rotation.  Filters [len x numChannels] or [len x numChannels x numSets]; 1 <= numListeners <= 4096;
% everything else as binauralDecodeStream.
    properties (SetAccess = private)
        handle = 0
        blockSize
        numSets
        numListeners
    end
    methods
        function g = binauralDecodeGroup(decodingFilterLeft, decodingFilterRight, blockSize, numListeners, shDefinition, rotationDomain, complexInput, encoder)
            if nargin < 5; shDefinition = 'real'; end
            if nargin < 6; rotationDomain = 'sh'; end
            if nargin < 7; complexInput = false; end
            if nargin < 8; encoder = []; end   % [numChannels x numMics]: the common block is one of real microphone signals (DESIGN.md 9.6)
            if isreal(decodingFilterLeft) ~= isreal(decodingFilterRight)
                decodingFilterLeft = complex(decodingFilterLeft); decodingFilterRight = complex(decodingFilterRight);
            end
            g.blockSize = blockSize;
            g.numSets = size(decodingFilterLeft, 3);
            g.numListeners = numListeners;
            g.handle = emagls_mex('group_create', double(decodingFilterLeft), double(decodingFilterRight), double(blockSize), ...
                                  double(numListeners), shDefinition, rotationDomain, logical(complexInput), double(encoder));
        end
        function out = push(g, block, horRotAngleRad, pitchRad, rollRad, setIndex)
            if nargin < 3; horRotAngleRad = []; end
            if nargin < 4; pitchRad = []; end
            if nargin < 5; rollRad = []; end
            if nargin < 6; setIndex = []; end
            out = emagls_mex('group_push', g.handle, double(block), double(horRotAngleRad), double(pitchRad), double(rollRad), ...
                             double(setIndex));
        end
        function reset(g, listener)
            if nargin < 2; listener = []; end
            emagls_mex('group_reset', g.handle, double(listener));
        end
        function delete(g)
            if g.handle > 0
                emagls_mex('group_destroy', g.handle);
                g.handle = 0;
            end
        end
    end
end
